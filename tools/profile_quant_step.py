#!/usr/bin/env python3
"""Rate control by quantisation step (csrc/quant_step.hip, DESIGN.md 4.7 "variable rate"): what the one-pass ladder cost launch
buys, what it is bound by, and what ``compress(target_bpp=...)`` costs on top of ``compress``.

    python tools/profile_quant_step.py [--out profiles/quant_step.json] [--reps 25]

Latents of an 18 x 512 x 768 batch at C = 320 ([18, 32, 48, 320] floats around mu, spread as their tables; scale indexes over all
64 tables).  Recorded:
  * ``sntc_step_ladder_cost`` at K = 16 against 16 x (``sntc_step_symbols`` + ``sntc_rans_cost``), the composition it replaces
    (same integers: asserted), and at K = 1, 4, 8 for the slope per candidate;
  * the K = 16 launch against its traffic, 10 bytes per element (y, mu, id) at the 6.3 TB/s a streaming read achieves;
  * ``Model.compress(x, target_bpp=...)`` against ``Model.compress(x)`` on the same images (host wall clock, synchronised).
Kernel figures: warm-up, then the median of ``reps`` runs between two HIP events on the launch stream, the variants alternating
inside one loop (output allocations included on both sides)."""
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
from shallow_ntc_amd import ops  # noqa: E402
from shallow_ntc_amd.common import data_lib  # noqa: E402
from shallow_ntc_amd.mshyper import configs  # noqa: E402
from shallow_ntc_amd.mshyper.models import Model  # noqa: E402

STREAM_TBS = 6.3          # achieved by a float4 streaming read on MI355X


def gpu_medians_ms(fns, reps, warmup=5):
    """Median time of each callable of ``fns`` (a dict), the callables alternating inside every repetition."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b))
    return {k: round(statistics.median(v), 4) for k, v in ts.items()}


def wall_medians_ms(fns, reps, warmup=2):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append(1e3 * (time.perf_counter() - t))
    return {k: round(statistics.median(v), 3) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "quant_step.json"))
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--images", type=int, default=18)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, h, w, c = args.images, 32, 48, 320
    rng = np.random.default_rng(0)
    ids = rng.integers(0, 64, size=(n, h, w, c))
    sig = 0.11 * np.exp(ec.SCALE_FACTOR * ids)
    mu = (2.0 * rng.standard_normal((n, h, w, c))).astype(np.float32)
    hyper = np.concatenate([mu, np.log(np.maximum(ids, 0.2)).astype(np.float32)], axis=-1)
    y = (mu + rng.standard_normal((n, h, w, c)) * sig).astype(np.float32)
    yd, hd = torch.from_numpy(y).to(dev), torch.from_numpy(hyper).to(dev)
    base = ec.scale_table_ids(hd)
    dt = ec.DeviceTables(ec.normal_tables(), dev)
    ladder = [-32, -24, -16, -12, -8, -6, -4, -2, 0, 2, 4, 6, 8, 12, 16, 32]
    tensors = {k: ec.step_tensors(ladder[:k], dev) for k in (1, 4, 8, 16)}
    per_image = [ec.step_tensors([k] * n, dev) for k in ladder]

    def composed():
        out = []
        for _, inv, sh in per_image:
            sym, tid = ops.step_symbols(yd, hd, base, inv, sh)
            out.append(ec.rans_cost(sym, tid, dt))
        return torch.stack(out, dim=1)

    one = ec.step_ladder_cost(yd, hd, base, ladder, dt, tensors[16])
    assert torch.equal(one, composed())
    elements = int(yd.numel())
    fns = {f"ladder_k{k}_ms": (lambda k=k: ec.step_ladder_cost(yd, hd, base, ladder[:k], dt, tensors[k])) for k in (1, 4, 8, 16)}
    fns["composed_16x_symbols_plus_cost_ms"] = composed
    fns["step_symbols_ms"] = lambda: ops.step_symbols(yd, hd, base, per_image[3][1], per_image[3][2])
    fns["scale_table_ids_ms"] = lambda: ec.scale_table_ids(hd)
    out = dict(device=torch.cuda.get_device_name(0), latents=[n, h, w, c], elements=elements, ladder=ladder,
               timer=f"median of {args.reps} after warm-up, variants alternating; launches: HIP events on the launch stream (output "
                     "allocations and the zeroing of the sums included); compress: host wall clock around a synchronised call")
    out["launches"] = gpu_medians_ms(fns, args.reps)
    t16 = out["launches"]["ladder_k16_ms"]
    out["ladder_k16_speedup_over_composed"] = round(out["launches"]["composed_16x_symbols_plus_cost_ms"] / t16, 2)
    traffic = 10 * elements
    out["ladder_k16_traffic_bytes"] = traffic
    out["ladder_k16_traffic_floor_ms"] = round(traffic / (STREAM_TBS * 1e12) * 1e3, 4)
    out["ladder_k16_tbs"] = round(traffic / (t16 * 1e-3) / 1e12, 3)
    out["ladder_k16_share_of_streaming_read"] = round(out["ladder_k16_tbs"] / STREAM_TBS, 3)
    out["ladder_lookups_per_ns"] = round(16 * elements / (t16 * 1e6), 2)       # one lookup = descriptor + price read from LDS
    print(json.dumps(out, indent=1), flush=True)

    model = Model(device=dev, **configs.two_layer_syn(rd_lambda=0.02))
    wts = dict(model.get_weights())
    b = wts["hyper_synthesis/layer_2/bias"].copy()
    b[c:] = np.random.default_rng(0).uniform(-1.0, 2.5, size=c)          # spread the scale indexes (random weights leave them at the floor)
    wts["hyper_synthesis/layer_2/bias"] = b.astype(np.float32)
    model.set_weights(wts)
    x = torch.from_numpy(data_lib.normalize_image(data_lib.synthetic_images(n, 512, 768, seed=11))).to(dev)
    plain = model.compress(x)
    codec = model._get_codec()
    lat = model.infer_latent_rvs(x)
    cz, cy = codec.ladder_cost(lat.uq[0].loc, lat.uq[1].loc, (512, 768), [0, 3])
    bits = (cz[:, None] + cy).cpu().numpy() / 65536.0 + codec.flushed_bits(512, 768)
    target = float(bits[:, 1].max() + 1.0) / (512 * 768)               # every image fits at k = 3, some at a finer step
    blob = model.compress(x, target_bpp=target)
    rep = model.last_compress_report
    r = dict(images=[n, 512, 768], plain_bytes=len(plain), plain_bpp=round(8 * len(plain) / (n * 512 * 768), 5), target_bpp=round(target, 5),
             target_bytes=len(blob), target_file_bpp=round(8 * len(blob) / (n * 512 * 768), 5),
             steps_chosen=[q["step_chosen"] for q in rep], met=[q["met"] for q in rep])
    r.update(wall_medians_ms({"compress_ms": lambda: model.compress(x), "compress_target_bpp_ms": lambda: model.compress(x, target_bpp=target),
                              "compress_step_ms": lambda: model.compress(x, step=r["steps_chosen"])}, max(8, args.reps // 3)))
    out["compress"] = r
    print(json.dumps(r, indent=1), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
