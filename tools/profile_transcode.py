#!/usr/bin/env python3
"""Transcoding a bitstream to a coarser step without pixels (csrc/quant_step.hip, DESIGN.md 4.7 "transcode"): what it costs
beside the round trip it replaces, what its launches take, and what the second rounding costs in rate and quality.

    python tools/profile_transcode.py [--out profiles/transcode.json] [--reps 15]

Recorded, on the Kodak-shaped set (18 images of 512 x 768 and 6 of 768 x 512, two blobs at ladder index 0):
  * ``Model.transcode_many(blobs, shift=d)`` against the path without it, ``decompress_many(blobs)`` followed by one
    ``compress(x, step=d)`` per batch of decoded pixels; ``transcode_many(blobs, target_bpp=...)`` beside them; and
    ``decompress_many`` alone, whose front half (z decode, hyper-synthesis, y decode) transcoding shares.  Host wall clock around
    a synchronised call, the variants alternating inside one loop: median, min and max of ``reps`` after warm-up, and the ratio
    of the medians;
  * the two new launches on the latents of the 18-image batch: ``sntc_step_requant_symbols`` and
    ``sntc_step_requant_ladder_cost`` at 16 shifts, beside the compositions they fuse (same integers: asserted), between two HIP
    events on the launch stream;
  * for d = 1, 2, 4, 8 from ladder index 0: bpp and PSNR of the transcoded file and of ``compress(x, step=d)`` from the original
    pixels (the reference of both columns), per shift over the 24 images -- the price of quantising twice."""
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
sys.path.insert(0, str(ROOT / "tools"))
import __graft_entry__ as graft  # noqa: E402

graft.load_package()
from profile_quant_step import gpu_medians_ms  # noqa: E402
from shallow_ntc_amd import entropy_coding as ec  # noqa: E402
from shallow_ntc_amd import ops  # noqa: E402
from shallow_ntc_amd.common import data_lib  # noqa: E402
from shallow_ntc_amd.mshyper import configs  # noqa: E402
from shallow_ntc_amd.mshyper.models import Model  # noqa: E402


def wall_stats_ms(fns, reps, warmup=3):
    """Median, min and max of each callable's synchronised wall time, the callables alternating inside every repetition."""
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
    return {k: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3)) for k, v in ts.items()}


def psnr(px, x):
    """PSNR in dB of uint8 pixels against normalised images, over the whole batch."""
    ref = torch.round((x.double() + 0.5) * 255.0)
    return float(ec.psnr_of_sse(float(((px.double() - ref) ** 2).sum().item()), x.numel()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "transcode.json"))
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model = Model(device=dev, **configs.two_layer_syn(rd_lambda=0.02))
    c = 320
    wts = dict(model.get_weights())
    b = wts["hyper_synthesis/layer_2/bias"].copy()
    b[c:] = np.random.default_rng(0).uniform(-1.0, 2.5, size=c)          # spread the scale indexes (random weights leave them at the floor)
    wts["hyper_synthesis/layer_2/bias"] = b.astype(np.float32)
    model.set_weights(wts)
    xs = [torch.from_numpy(data_lib.normalize_image(data_lib.synthetic_images(n, h, w, seed=11 + n))).to(dev)
          for n, h, w in ((18, 512, 768), (6, 768, 512))]
    pixels = sum(int(x.shape[0] * x.shape[1] * x.shape[2]) for x in xs)
    blobs = [model.compress(x) for x in xs]
    assert [bl[4] for bl in blobs] == [3, 3]
    d = 4

    def round_trip(k=d):
        return [model.compress(px.float() / 255.0 - 0.5, step=k) for px in model.decompress_many(blobs)]

    out = dict(device=torch.cuda.get_device_name(0), images=[[int(v) for v in x.shape[:3]] for x in xs], source_bytes=[len(bl) for bl in blobs],
               shift=d, timer=f"host wall clock around a synchronised call, variants alternating in one loop: median / min / max of "
                              f"{args.reps} after 3 warm-up rounds; launches: median between two HIP events on the launch stream")
    got, via = model.transcode_many(blobs, shift=d), round_trip()
    out["bytes"] = dict(transcode=[len(v) for v in got], decompress_then_compress=[len(v) for v in via])
    target = [8.0 * len(v) / float(x.shape[0] * x.shape[1] * x.shape[2]) for v, x in zip(got, xs)]
    out["calls"] = wall_stats_ms({"transcode_many_shift": lambda: model.transcode_many(blobs, shift=d),
                                  "transcode_many_target_bpp": lambda: model.transcode_many(blobs, target_bpp=target),
                                  "decompress_many_then_compress_step": round_trip,
                                  "decompress_many": lambda: model.decompress_many(blobs)}, args.reps)
    med = lambda k: out["calls"][k]["median_ms"]
    out["round_trip_over_transcode"] = round(med("decompress_many_then_compress_step") / med("transcode_many_shift"), 2)
    out["transcode_share_of_decompress_many"] = round(med("transcode_many_shift") / med("decompress_many"), 2)
    out["target_bpp_shifts"] = [[r["step_chosen"] for r in rep] for rep in model.last_compress_report]
    print(json.dumps(out, indent=1), flush=True)

    # the two launches, on what the 18-image blob holds
    codec = model._get_codec()
    lat = model.infer_latent_rvs(xs[0])
    z, y = lat.uq[0].loc.contiguous(), lat.uq[1].loc.contiguous()
    n = int(y.shape[0])
    _, _, sym, _, hyper = codec._symbols(z, y, ec.StepGrid("unit", n))
    base, lut = ec.scale_table_ids(hyper), ec.cached_step_lut(dev)
    src = torch.zeros(tuple(y.shape[:3]), dtype=torch.int8, device=dev)
    dst = torch.full_like(src, d)
    shifts = list(range(16))
    shifts_d = torch.tensor(shifts, dtype=torch.int32).to(dev)
    cost = torch.empty((n, 16), dtype=torch.int64, device=dev)

    def composed_symbols():
        return ops.step_map_symbols(ops.dequant_step_map(sym, hyper, src, lut), hyper, base, dst, lut)

    def composed_cost():
        return ec.step_map_ladder_cost(ops.dequant_step_map(sym, hyper, src, lut), hyper, base, src, shifts, codec.y_tables, lut, shifts_d)

    a, bb = ops.step_requant_symbols(sym, hyper, base, src, dst, lut), composed_symbols()
    assert torch.equal(a[0], bb[0]) and torch.equal(a[1], bb[1])
    assert torch.equal(ops.step_requant_ladder_cost(sym, hyper, base, src, lut, shifts_d, codec.y_tables, out=cost), composed_cost())
    elements = int(sym.numel())
    out["launches"] = dict(latents=[int(v) for v in sym.shape], elements=elements, **gpu_medians_ms({
        "requant_symbols_ms": lambda: ops.step_requant_symbols(sym, hyper, base, src, dst, lut),
        "dequant_map_plus_map_symbols_ms": composed_symbols,
        "requant_ladder_cost_k16_ms": lambda: ops.step_requant_ladder_cost(sym, hyper, base, src, lut, shifts_d, codec.y_tables, out=cost),
        "dequant_map_plus_map_ladder_cost_k16_ms": composed_cost}, max(25, args.reps)))
    t = out["launches"]["requant_symbols_ms"]
    out["launches"]["requant_symbols_tbs"] = round(16 * elements / (t * 1e-3) / 1e12, 3)          # 4 + 4 + 2 read, 4 + 2 written per element
    print(json.dumps(out["launches"], indent=1), flush=True)

    # rate and quality: the transcoded file beside compress(x, step=d) from the original pixels, from ladder index 0
    rows = []
    for k in (1, 2, 4, 8):
        twice, direct = model.transcode_many(blobs, shift=k), [model.compress(x, step=k) for x in xs]
        px_t, px_d = model.decompress_many(twice), model.decompress_many(direct)
        sse = lambda pxs: sum(float(((p.double() - torch.round((x.double() + 0.5) * 255.0)) ** 2).sum().item()) for p, x in zip(pxs, xs))
        rows.append(dict(shift=k, transcode_bpp=round(8.0 * sum(len(v) for v in twice) / pixels, 5),
                         direct_bpp=round(8.0 * sum(len(v) for v in direct) / pixels, 5),
                         transcode_psnr=round(float(ec.psnr_of_sse(sse(px_t), 3 * pixels)), 4),
                         direct_psnr=round(float(ec.psnr_of_sse(sse(px_d), 3 * pixels)), 4)))
        rows[-1]["bpp_ratio"] = round(rows[-1]["transcode_bpp"] / rows[-1]["direct_bpp"], 4)
        rows[-1]["psnr_loss_db"] = round(rows[-1]["direct_psnr"] - rows[-1]["transcode_psnr"], 4)
    px0 = model.decompress_many(blobs)
    out["source"] = dict(bpp=round(8.0 * sum(len(v) for v in blobs) / pixels, 5), psnr=round(sum(psnr(p, x) * x.shape[0] for p, x in zip(px0, xs)) / 24.0, 4),
                         note="psnr: mean of the two batches' PSNR weighted by images; the rows below pool the squared error of all 24")
    out["double_quantisation"] = rows
    out["model"] = "two_layer_syn, seeded random weights with spread scale biases, synthetic images: the comparison between the two " \
                   "columns is what is measured, not the codec's operating point"
    print(json.dumps(rows, indent=1), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
