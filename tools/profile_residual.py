#!/usr/bin/env python3
"""The coded pixel residual layer (csrc/residual.hip, wire format 8, DESIGN.md 4.7 "residual layer"): what its kernels, its
streams and the calls around them take, and what the layer costs in the file.

    python tools/profile_residual.py [--out profiles/residual.json] [--reps 15]

Recorded, on the Kodak-shaped synthetic set (18 images of 512 x 768 and 6 of 768 x 512):
  * the three kernels on the 18-image batch against their algorithmic traffic (quantize 4 + 1 in, 4 out; table ids 1 in, 2 out;
    apply 1 + 4 in, 1 out bytes per value), median between two HIP events, the variants alternating inside one loop -- the
    quantiser also on a SMOOTH picture (constant x over a constant base: every value of a channel hits one LDS counter);
  * the residual streams' entropy decode alone, per blob (``rans_decode`` of the layer's words between two HIP events);
  * ``compress`` and ``decompress_many`` with and without the layer, and ``decompress_many`` of the plain blobs on its own
    (median, min and max: the spread a comparison with another commit has to be read against), host wall clock around a
    synchronised call, the variants alternating;
  * the layer's bits per pixel at max_error 0, 1, 2, 4 beside the base's, and the worst pixel error of each file."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import __graft_entry__ as graft  # noqa: E402

graft.load_package()
from profile_quant_step import gpu_medians_ms  # noqa: E402
from profile_transcode import wall_stats_ms  # noqa: E402
from shallow_ntc_amd import entropy_coding as ec  # noqa: E402
from shallow_ntc_amd.common import data_lib  # noqa: E402
from shallow_ntc_amd.mshyper import configs  # noqa: E402
from shallow_ntc_amd.mshyper.models import Model  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "residual.json"))
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model = Model(device=dev, **configs.two_layer_syn(rd_lambda=0.02))
    wts = dict(model.get_weights())
    b = wts["hyper_synthesis/layer_2/bias"].copy()
    b[320:] = np.random.default_rng(0).uniform(-1.0, 2.5, size=320)      # spread the scale indexes (random weights leave them at the floor)
    wts["hyper_synthesis/layer_2/bias"] = b.astype(np.float32)
    model.set_weights(wts)
    codec = model._get_codec()
    xs = [torch.from_numpy(data_lib.normalize_image(data_lib.synthetic_images(n, h, w, seed=11 + n))).to(dev)
          for n, h, w in ((18, 512, 768), (6, 768, 512))]
    pixels = sum(int(x.shape[0] * x.shape[1] * x.shape[2]) for x in xs)
    plain = [model.compress(x) for x in xs]
    delta = 2
    layered = [model.compress(x, max_error=delta) for x in xs]
    out = dict(device=torch.cuda.get_device_name(0), images=[[int(v) for v in x.shape[:3]] for x in xs], max_error=delta,
               timer="kernels and stream decode: median between two HIP events on the launch stream, variants alternating; calls: host "
                     f"wall clock around a synchronised call, variants alternating: median / min / max of {args.reps} after 3 warm-up rounds",
               model="two_layer_syn, seeded random weights with spread scale biases, synthetic images: the figures say that the path "
                     "runs and what it costs on THIS model; nothing is claimed for trained weights")

    # the three kernels on the 18-image batch
    x = xs[0]
    base = model.decompress(plain[0])
    elements = int(base.numel())
    q, hist = ec.residual_quantize(x, base, delta)
    choice, _ = ec.residual_choice(hist.cpu().numpy().view(np.uint32), codec.y_tables.host)
    choice_d = torch.from_numpy(choice).to(dev)
    smooth_x, smooth_b = torch.zeros_like(x), torch.full_like(base, 128)
    reps = max(25, args.reps)
    k = gpu_medians_ms({"quantize_ms": lambda: ec.residual_quantize(x, base, delta),
                        "quantize_lossless_ms": lambda: ec.residual_quantize(x, base, 0),
                        "quantize_smooth_ms": lambda: ec.residual_quantize(smooth_x, smooth_b, delta),
                        "table_ids_ms": lambda: ec.residual_table_ids(base, choice_d),
                        "apply_ms": lambda: ec.residual_apply(base, q, delta)}, reps)
    tbs = lambda bytes_per, ms: round(bytes_per * elements / (ms * 1e-3) / 1e12, 3)
    out["kernels"] = dict(elements=elements, **k, quantize_tbs=tbs(9, k["quantize_ms"]), quantize_smooth_tbs=tbs(9, k["quantize_smooth_ms"]),
                          table_ids_tbs=tbs(3, k["table_ids_ms"]), apply_tbs=tbs(6, k["apply_ms"]),
                          note="each time includes the kernel that zeroes the histogram / the counter in front of the launch")
    print(json.dumps(out["kernels"], indent=1), flush=True)

    # the residual streams' decode alone, per blob
    rows = []
    for bl in layered:
        base_blob, info = ec.split_residual(bl)
        bpx = model.decompress(base_blob)
        ids = ec.residual_table_ids(bpx, torch.from_numpy(info["choice"].copy()).to(dev))
        words = torch.from_numpy(np.frombuffer(bl, "<i2", info["words"], info["pos"]).copy()).to(dev)
        offs = torch.from_numpy(np.concatenate([[0], np.cumsum(info["lens"])]).astype(np.int64)).to(dev)
        bad = torch.zeros((1,), dtype=torch.int32, device=dev)
        shape = (info["n"], info["H"], info["W"], 3)
        fn = lambda: ec.rans_decode(words, info["lens"], ids, shape, codec.y_tables, info["segments"], info["lanes"], bad=bad, offsets=offs)
        t = gpu_medians_ms({"ms": fn}, reps)["ms"]
        assert int(bad.item()) == 0
        rows.append(dict(images=list(shape[:3]), streams=info["n"] * info["segments"], steps_per_stream=-(-shape[1] * shape[2] * 3 // info["segments"] // 64),
                         decode_ms=t, us_per_step=round(1e3 * t / (-(-shape[1] * shape[2] * 3 // info["segments"] // 64)), 3)))
    out["stream_decode"] = rows
    print(json.dumps(rows, indent=1), flush=True)

    # the calls
    out["compress"] = wall_stats_ms({"plain": lambda: [model.compress(v) for v in xs],
                                     "max_error": lambda: [model.compress(v, max_error=delta) for v in xs]}, args.reps)
    out["decompress_many"] = wall_stats_ms({"plain": lambda: model.decompress_many(plain),
                                            "max_error": lambda: model.decompress_many(layered)}, args.reps)
    out["decompress_many_plain_alone"] = wall_stats_ms({"plain": lambda: model.decompress_many(plain)}, 2 * args.reps)["plain"]
    print(json.dumps({k: out[k] for k in ("compress", "decompress_many", "decompress_many_plain_alone")}, indent=1), flush=True)

    # what the layer costs in the file
    x8 = [torch.round((v.double() + 0.5) * 255.0).clamp(0, 255).to(torch.int32) for v in xs]
    worst = lambda pxs: max(int((p.to(torch.int32) - r).abs().max().item()) for p, r in zip(pxs, x8))
    rate = [dict(file="base", bpp=round(8.0 * sum(len(v) for v in plain) / pixels, 4), worst_pixel_error=worst(model.decompress_many(plain)))]
    for d in (0, 1, 2, 4):
        files = [model.add_residual(bl, v, d) for bl, v in zip(plain, xs)]
        layer_bytes = sum(len(f) - len(bl) for f, bl in zip(files, plain))
        pred = sum(float(model.residual_bits(v, bl, d).sum()) for bl, v in zip(plain, xs))
        rate.append(dict(file=f"max_error {d}", layer_bpp=round(8.0 * layer_bytes / pixels, 4), layer_bits_per_value=round(8.0 * layer_bytes / (3 * pixels), 4),
                         predicted_layer_bpp=round(pred / pixels, 4), total_bpp=round(8.0 * sum(len(f) for f in files) / pixels, 4),
                         worst_pixel_error=worst(model.decompress_many(files))))
        assert rate[-1]["worst_pixel_error"] <= d
    out["rate"] = rate
    print(json.dumps(rate, indent=1), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
