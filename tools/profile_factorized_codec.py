#!/usr/bin/env python3
"""Entropy coding of the factorized-prior model's latents: the channel-indexed launches (csrc/rans_channels.hip) against the
composition of entry points they replace, and compress / decompress wall time of factorized.Model at the reference's width.

    python tools/profile_factorized_codec.py [--out profiles/factorized_codec.json] [--reps 25]

Latents of an 18 x 512 x 768 batch and of one 512 x 768 image at C = 256 ([n, 32, 48, 256] floats drawn around each channel's
table).  Composed = round_to_int + channel_table_ids + rans_encode, and channel_table_ids + rans_decode + int_to_float -- what
Codec does for the hyper-latents.  Every figure: warm-up, then the median of ``reps`` runs between two HIP events on the launch
stream (allocations of the outputs included on both sides); compress / decompress: host wall clock around a synchronised call."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as graft  # noqa: E402

graft.load_package()
from shallow_ntc_amd import entropy_coding as ec  # noqa: E402
from shallow_ntc_amd.common import data_lib  # noqa: E402
from shallow_ntc_amd.factorized.models import Model  # noqa: E402
from shallow_ntc_amd.mshyper.models import deep_factorized_init  # noqa: E402


def gpu_median_ms(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return round(statistics.median(ts), 4)


def wall_median_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t))
    return round(statistics.median(ts), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "factorized_codec.json"))
    ap.add_argument("--reps", type=int, default=25)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    C = 256
    rng = np.random.default_rng(0)
    pw = {k: (v + 0.3 * rng.standard_normal(v.shape)).astype(np.float32) for k, v in deep_factorized_init(C, (3, 3, 3)).items()}
    tabs = ec.factorized_tables(pw, 4)
    dt = ec.DeviceTables(tabs, dev)
    lo = np.array([t[0] for t in tabs])
    width = np.array([len(t[1]) - 1 for t in tabs])
    out = dict(device=torch.cuda.get_device_name(0), channels=C, table_entries=dt.total, start_tables_resident=dt.dec is not None,
               timer=f"median of {args.reps} after warm-up; launches: HIP events on the launch stream; compress / decompress: host wall clock",
               shapes={})
    for n in (18, 1):
        shape = (n, 32, 48, C)
        y = (lo + width // 2 + rng.laplace(0, 1, size=shape) * np.maximum(width / 12.0, 0.6)).astype(np.float32)
        yd = torch.from_numpy(y).to(dev)
        payload, lens, _ = ec.rans_encode_channels(yd, dt)
        old_payload, old_lens = ec.rans_encode(ec.round_to_int(yd), ec.channel_table_ids(shape, dev), dt)
        assert torch.equal(payload, old_payload) and lens.tolist() == old_lens.tolist()
        offs = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(dev)
        bad = torch.zeros((1,), dtype=torch.int32, device=dev)
        r = dict(elements=int(yd.numel()), streams=len(lens), payload_bytes=2 * int(lens.sum()))
        r["encode_composed_ms"] = gpu_median_ms(lambda: ec.rans_encode_launch(ec.round_to_int(yd), ec.channel_table_ids(shape, dev), dt), args.reps)
        r["encode_fused_ms"] = gpu_median_ms(lambda: ec.rans_encode_channels_launch(yd, dt), args.reps)
        r["decode_composed_ms"] = gpu_median_ms(lambda: ec.int_to_float(ec.rans_decode(payload, lens, ec.channel_table_ids(shape, dev), shape, dt,
                                                                                        bad=bad, offsets=offs)), args.reps)
        r["decode_fused_ms"] = gpu_median_ms(lambda: ec.rans_decode_channels(payload, lens, shape, dt, bad=bad, offsets=offs), args.reps)
        assert int(bad.item()) == 0
        assert torch.equal(ec.rans_decode_channels(payload, lens, shape, dt), torch.from_numpy(np.rint(y)).to(dev))
        out["shapes"][f"{n}x512x768"] = r
        print(n, r, flush=True)
    tc = dict(analysis=dict(cls="BLS2017Analysis", num_filters=C), synthesis=dict(cls="BLS2017Synthesis", num_filters=C))
    model = Model(device=dev, rd_lambda=0.02, transform_config=tc)
    w = dict(model.get_weights())
    for k in w:
        if k.startswith("prior/"):
            w[k] = (w[k] + 0.3 * rng.standard_normal(w[k].shape)).astype(np.float32)
    probe = torch.from_numpy(data_lib.normalize_image(data_lib.synthetic_images(1, 128, 192, seed=3))).to(dev)
    w["analysis/layer_2/kernel"] = (w["analysis/layer_2/kernel"] * (3.0 / float(model.infer_latent_rvs(probe).uq[0].loc.std()))).astype(np.float32)
    model.set_weights(w)
    for n in (18, 1):
        x = torch.from_numpy(data_lib.normalize_image(data_lib.synthetic_images(n, 512, 768, seed=11))).to(dev)
        blob = model.compress(x)
        r = out["shapes"][f"{n}x512x768"]
        r["model_blob_bytes"] = len(blob)
        r["model_bpp"] = round(8 * len(blob) / (n * 512 * 768), 4)
        r["model_estimate_ratio"] = round(8 * len(blob) / float(model.encode(x)[3].sum()), 4)
        r["compress_wall_ms"] = wall_median_ms(lambda: model.compress(x), max(10, args.reps // 2))
        r["decompress_wall_ms"] = wall_median_ms(lambda: model.decompress(blob), max(10, args.reps // 2))
        print(n, r, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
