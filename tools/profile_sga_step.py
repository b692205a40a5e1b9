#!/usr/bin/env python3
"""SGA iterative inference at a quantisation step (csrc/sga.hip ``sga_normal_step_*``).

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/profile_sga_step.py kernels
    python tools/profile_sga_step.py compress [--out profiles/sga_step.json] [--steps 100]
    python tools/profile_sga_step.py map [--out profiles/sga_step_map.json] [--steps 100]

``kernels``: the kernel pairs of step 1 and of a step on 18 x 32 x 48 x 320 latents at ladder index 0 (the same arithmetic on the
same numbers: what differs is the layout), alternating, 30 calls each after 3 of warm-up, to be read from a kernel trace taken in
a run of its own (prints the bytes each launch moves).
``compress``: ``compress(x, itinf=dict(steps, step=k))`` for k in (-6, 0, +6) on the tests' fixture (2 x 128 x 128) and on one
512 x 768 image, ``two_layer_syn`` with spread scale biases and RANDOM weights: J_start -> J_chosen, bits, and the wall clock
against ``compress(x, step=k)``.
``map``: SGA on a step map (``sga_normal_step_map_*``, ``distortion_grad_weighted``, ``block_sse``) next to the uniform-step path, on
the same two image sets: the uniform path is ``step=-6``, the map is -6 on the centred half-size rectangle of positions and +6
around it (``step=-6`` with offsets 0 / +12).  Per SGA step (``itinf_train_step(fetch=False)``, synchronised host wall clock, the two
variants alternating on two models of the same weights, median of ``--calls``) and per ``compress(x, itinf=...)`` call (median of 3,
alternating).  RANDOM weights: the times are what is measured, not a rate-distortion gain."""
import argparse
import json
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


def kernels(args):
    dev = torch.device("cuda:0")
    n, h, w, c = 18, 32, 48, 320
    rng = np.random.default_rng(0)
    mu = (2.0 * rng.standard_normal((n, h, w, c))).astype(np.float32)
    raw = rng.uniform(-2.5, 4.5, size=mu.shape).astype(np.float32)
    ks = [args.k] * n            # ladder index 0: both pairs do the same arithmetic on the same numbers, only the layout differs
    y = (mu + np.float32(ec.step_size(args.k)) * rng.laplace(0, 2, size=mu.shape)).astype(np.float32)
    yd, hd = torch.from_numpy(y).to(dev), torch.from_numpy(np.concatenate([mu, raw], -1)).to(dev)
    g = torch.from_numpy(rng.standard_normal(mu.shape).astype(np.float32)).to(dev)
    quant = tuple(ec.step_tensors(ks, dev)) + (torch.ones(n, device=dev),)
    wgt = 1.0 / (n * 512 * 768)
    for i in range(args.calls + 3):
        old = ops.sga_normal_fwd(yd, hd, 0.4, None, 1, i)
        new = ops.sga_normal_step_fwd(yd, hd, 0.4, quant, None, 1, i)
        ops.sga_normal_bwd(g, old[1], old[2], old[3], wgt)
        ops.sga_normal_step_bwd(g, new[1], new[2], new[3], wgt, quant)
    torch.cuda.synchronize()
    e = yd.numel()
    print(json.dumps(dict(latents=[n, h, w, c], k=args.k, elements=e, calls=args.calls + 3, fwd_bytes=28 * e, bwd_bytes=28 * e,
                          note="fwd: y 4 + (mu, raw) 8 in, four outputs 16 out (generator noise); bwd: four inputs 16 in, g_y 4 + g_hyper 8 out")))
    return 0


def spread_model(dev):
    model = Model(device=dev, **{**configs.two_layer_syn(rd_lambda=0.02), **configs.itinf()})
    wts = dict(model.get_weights())
    b = wts["hyper_synthesis/layer_2/bias"].copy()
    b[320:] = np.random.default_rng(0).uniform(-1.0, 2.5, size=320)
    wts["hyper_synthesis/layer_2/bias"] = b.astype(np.float32)
    model.set_weights(wts)
    return model


def wall_ms(fn, reps=3):
    best = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        d = 1e3 * (time.perf_counter() - t)
        best = d if best is None else min(best, d)
    return round(best, 2)


def compress(args):
    dev = torch.device("cuda:0")
    model = spread_model(dev)
    out = dict(device=torch.cuda.get_device_name(0), weights="RANDOM (two_layer_syn, spread scale biases): what refinement buys on a "
               "trained model across the ladder is not measured here", steps=args.steps, timer="host wall clock, synchronised, best of 3",
               cases=[])
    sets = {"fixture 2x128x128": torch.from_numpy(data_lib.normalize_image(data_lib.synthetic_images(2, 128, 128, seed=21))).to(dev),
            "1x512x768": torch.from_numpy(data_lib.normalize_image(data_lib.synthetic_images(1, 512, 768, seed=11))).to(dev)}
    for name, x in sets.items():
        for k in (-6, 0, 6):
            itinf = dict(steps=args.steps, seed=3, step=k)
            model.compress(x, itinf=itinf)
            rep = model.last_compress_report
            row = dict(images=name, k=k, lam=rep[0]["lam"], step_chosen=[r["step_chosen"] for r in rep],
                       J_start=[round(r["J_start"], 6) for r in rep], J_chosen=[round(r["J_chosen"], 6) for r in rep],
                       bits_start=[r["bits_start"] for r in rep], bits_chosen=[r["bits_chosen"] for r in rep],
                       compress_itinf_ms=wall_ms(lambda: model.compress(x, itinf=itinf)),
                       compress_step_ms=wall_ms(lambda: model.compress(x, step=k)))
            out["cases"].append(row)
            print(json.dumps(row), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)
    return 0


def centred_offsets(model, n, H, W, inside=0, outside=12):
    h, w = model.step_offsets_shape(H, W)
    off = np.full((n, h, w), outside, np.int8)
    off[:, h // 4:h // 4 + h // 2, w // 4:w // 4 + w // 2] = inside
    return off


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)


def step_map(args):
    dev = torch.device("cuda:0")
    models = dict(uniform=spread_model(dev), map=spread_model(dev))      # the same weights twice: each keeps its own SGA state
    out = dict(device=torch.cuda.get_device_name(0), weights="RANDOM (two_layer_syn, spread scale biases): no rate-distortion gain on a "
               "trained model is claimed or measured here", steps=args.steps, base_step=-6,
               map="K = -6 on the centred half-size rectangle of positions, +6 around it (step=-6, offsets 0 / +12)",
               timer=f"host wall clock, synchronised; the two variants alternate; SGA step: median of {args.calls} after 3 of warm-up; "
                     "compress(itinf): median of 3 after one warm-up call", cases=[])
    sets = {"fixture 2x128x128": torch.from_numpy(data_lib.normalize_image(data_lib.synthetic_images(2, 128, 128, seed=21))).to(dev),
            "1x512x768": torch.from_numpy(data_lib.normalize_image(data_lib.synthetic_images(1, 512, 768, seed=11))).to(dev)}
    for name, x in sets.items():
        n, H, W = x.shape[0], x.shape[1], x.shape[2]
        off = centred_offsets(models["map"], n, H, W)
        kw = dict(uniform=dict(step=-6), map=dict(step=-6, step_offsets=off))
        for which, model in models.items():
            model.initialize_itinf(x, **kw[which])
        assert models["map"]._itinf_grid["grid"].kind == "map" and models["uniform"]._itinf_grid["grid"].kind == "image"
        times = dict(uniform=[], map=[])
        for i in range(args.calls + 3):
            for which, model in models.items():
                d = timed(lambda: model.itinf_train_step(x, seed=3, fetch=False))
                if i >= 3:
                    times[which].append(d)
        row = dict(images=name, positions=list(off.shape[1:]), inside=int((off[0] == 0).sum()),
                   sga_step_ms={k: round(float(np.median(v)), 3) for k, v in times.items()},
                   sga_step_ms_min_max={k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()})
        itinf = {k: dict(steps=args.steps, seed=3, **v) for k, v in kw.items()}
        times = dict(uniform=[], map=[])
        for i in range(4):
            for which, model in models.items():
                d = timed(lambda: model.compress(x, itinf=itinf[which]))
                if i >= 1:
                    times[which].append(d)
        row["compress_itinf_ms"] = {k: round(float(np.median(v)), 2) for k, v in times.items()}
        for which, model in models.items():
            rep = model.last_compress_report
            row[which] = dict(step_chosen=[r["step_chosen"] for r in rep], J_start=[round(r["J_start"], 6) for r in rep],
                              J_chosen=[round(r["J_chosen"], 6) for r in rep], bits_start=[r["bits_start"] for r in rep],
                              bits_chosen=[r["bits_chosen"] for r in rep])
        out["cases"].append(row)
        print(json.dumps(row), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernels", "compress", "map"])
    ap.add_argument("--out", default=None, help="default: profiles/sga_step.json (compress), profiles/sga_step_map.json (map)")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--k", type=int, default=0, help="kernels: the ladder index of every image")
    args = ap.parse_args()
    if args.out is None:
        args.out = str(ROOT / "profiles" / ("sga_step_map.json" if args.mode == "map" else "sga_step.json"))
    return dict(kernels=kernels, compress=compress, map=step_map)[args.mode](args)


if __name__ == "__main__":
    sys.exit(main())
