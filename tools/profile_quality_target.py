#!/usr/bin/env python3
"""Quality-targeted compress (csrc/quant_step.hip, DESIGN.md 4.7 "quality target"): what the ladder-dequantisation launch
is bound by, what decoding the candidates as batches buys over one ``coded_cost`` per step, and what
``compress(target_psnr=...)`` costs beside ``compress(target_bpp=...)``.

    python tools/profile_quality_target.py [--out profiles/quality_target.json] [--reps 25]

Recorded:
  * ``sntc_step_ladder_dequant`` at K = 16 on [18, 32, 48, 320] latents against its traffic, 8 bytes read and 4 K written per
    element, and against 16 x (``sntc_step_symbols`` + ``sntc_dequant_step``), the composition it replaces (same bits:
    asserted); K = 1, 4, 8 for the slope per candidate; the map kernel at K = 16;
  * ``Model.rd_curve`` of ONE 512 x 768 image on the whole ladder against the loop of 65 ``coded_cost(x, step=k)`` calls (same
    integers: asserted), and of the 18-image batch;
  * ``Model.compress(x, target_psnr=...)`` beside ``compress(x, target_bpp=...)`` and ``compress(x)``, one image and 18.
Kernel figures: warm-up, then the median of ``reps`` runs between two HIP events on the launch stream, the variants alternating
inside one loop (the output tensor is allocated once, outside).  Calls of the model: host wall clock around a synchronised call."""
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
from profile_quant_step import gpu_medians_ms, wall_medians_ms  # noqa: E402
from shallow_ntc_amd import entropy_coding as ec  # noqa: E402
from shallow_ntc_amd import ops  # noqa: E402
from shallow_ntc_amd.common import data_lib  # noqa: E402
from shallow_ntc_amd.mshyper import configs  # noqa: E402
from shallow_ntc_amd.mshyper.models import Model  # noqa: E402

WRITE_TBS = 6.3           # HBM bandwidth a streaming kernel achieves on MI355X (8 TB/s peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "quality_target.json"))
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
    ladder = [-32, -24, -16, -12, -8, -6, -4, -2, 0, 2, 4, 6, 8, 12, 16, 32]
    tensors = {k: ec.step_tensors(ladder[:k], dev) for k in (1, 4, 8, 16)}
    per_image = [ec.step_tensors([k] * n, dev) for k in ladder]
    out16 = torch.empty((16, n, h, w, c), dtype=torch.float32, device=dev)
    lut = ec.step_lut(dev)
    bases = torch.tensor(ladder, dtype=torch.int32).to(dev)
    offs = torch.from_numpy(rng.integers(-8, 9, size=(n, h, w)).astype(np.int8)).to(dev)

    def composed():
        return [ops.dequant_step(ops.step_symbols(yd, hd, base, inv, sh)[0], hd, st) for st, inv, sh in per_image]

    one = ops.step_ladder_dequant(yd, hd, tensors[16][1], tensors[16][0], out=out16)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(one, composed()))
    elements = int(yd.numel())
    fns = {f"ladder_dequant_k{k}_ms": (lambda k=k: ops.step_ladder_dequant(yd, hd, tensors[k][1], tensors[k][0], out=out16[:k]))
           for k in (1, 4, 8, 16)}
    fns["map_ladder_dequant_k16_ms"] = lambda: ops.step_map_ladder_dequant(yd, hd, offs, lut, bases, out=out16)
    fns["composed_16x_symbols_plus_dequant_ms"] = composed
    out = dict(device=torch.cuda.get_device_name(0), latents=[n, h, w, c], elements=elements, ladder=ladder,
               timer=f"median of {args.reps} after warm-up, variants alternating; launches: HIP events on the launch stream (the ladder "
                     "kernels write a tensor allocated once; the composition allocates its own); model calls: host wall clock around a "
                     "synchronised call")
    out["launches"] = gpu_medians_ms(fns, args.reps)
    for name in ("ladder_dequant_k16", "map_ladder_dequant_k16"):
        t = out["launches"][name + "_ms"]
        traffic = (8 + 4 * 16) * elements
        out[name] = dict(us=round(1e3 * t, 1), traffic_bytes=traffic, written_bytes=64 * elements,
                         tbs=round(traffic / (t * 1e-3) / 1e12, 3), written_tbs=round(64 * elements / (t * 1e-3) / 1e12, 3),
                         traffic_floor_us=round(traffic / (WRITE_TBS * 1e12) * 1e6, 1),
                         share_of_streaming_bandwidth=round(traffic / (t * 1e-3) / 1e12 / WRITE_TBS, 3))
    out["ladder_dequant_k16_speedup_over_composed"] = round(out["launches"]["composed_16x_symbols_plus_dequant_ms"] /
                                                            out["launches"]["ladder_dequant_k16_ms"], 2)
    print(json.dumps(out, indent=1), flush=True)
    del out16, one

    model = Model(device=dev, **configs.two_layer_syn(rd_lambda=0.02))
    wts = dict(model.get_weights())
    b = wts["hyper_synthesis/layer_2/bias"].copy()
    b[c:] = np.random.default_rng(0).uniform(-1.0, 2.5, size=c)          # spread the scale indexes (random weights leave them at the floor)
    wts["hyper_synthesis/layer_2/bias"] = b.astype(np.float32)
    model.set_weights(wts)
    x = torch.from_numpy(data_lib.normalize_image(data_lib.synthetic_images(n, 512, 768, seed=11))).to(dev)
    whole = list(range(ec.STEP_MIN, ec.STEP_MAX + 1))
    reps = max(5, args.reps // 5)
    out["model"] = {}
    for name, xs in (("one_image", x[:1]), (f"{n}_images", x)):
        def loop(xs=xs):
            return np.stack([model.coded_cost(xs, step=k)["sse"] for k in whole], axis=1)

        rd = model.rd_curve(xs)
        r = dict(images=[int(xs.shape[0]), 512, 768], candidates=len(whole))
        if xs.shape[0] == 1:
            assert rd["sse"].tolist() == loop().astype(np.int64).tolist()
            r.update(wall_medians_ms({"rd_curve_ms": lambda xs=xs: model.rd_curve(xs), "loop_of_65_coded_cost_ms": loop}, reps))
            r["speedup"] = round(r["loop_of_65_coded_cost_ms"] / r["rd_curve_ms"], 2)
        else:
            r.update(wall_medians_ms({"rd_curve_ms": lambda xs=xs: model.rd_curve(xs)}, reps))
        r["rd_curve_ms_per_image_and_candidate"] = round(r["rd_curve_ms"] / (xs.shape[0] * len(whole)), 4)
        # targets every image can meet: the curve's value at k = 3, per image (a hair below: the budget is a float of its own)
        q = [float(v) - 1e-6 for v in rd["psnr"][:, whole.index(3)]]
        bpp = [float(v) + 1e-9 for v in rd["bpp"][:, whole.index(3)]]
        blob = model.compress(xs, target_psnr=q)
        rep = model.last_compress_report
        r.update(target_psnr_steps=[t["step_chosen"] for t in rep], target_psnr_met=[t["met"] for t in rep], target_psnr_bytes=len(blob))
        r.update(wall_medians_ms({"compress_ms": lambda xs=xs: model.compress(xs),
                                  "compress_target_bpp_ms": lambda xs=xs: model.compress(xs, target_bpp=bpp),
                                  "compress_target_psnr_ms": lambda xs=xs: model.compress(xs, target_psnr=q)}, reps))
        out["model"][name] = r
        print(json.dumps(r, indent=1), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
