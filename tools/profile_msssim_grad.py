#!/usr/bin/env python3
"""(MS-)SSIM as a differentiable distortion (csrc/msssim_grad.hip): what value + gradient cost next to the
forward-only metric, each new kernel against its algorithmic traffic, and the SGA step under "mse" and "ms_ssim".

    python tools/profile_msssim_grad.py [--out profiles/msssim_grad.json] [--reps 25]

Shapes 5 x 1200 x 1200 x 3, 18 x 512 x 768 x 3 and 1 x 512 x 768 x 3.  Every figure: warm-up, then the median of ``reps`` runs
between two HIP events on the launch stream (output allocations included).  Algorithmic traffic of a gradient launch: read a
and b, read the coarser gradient, write g; of the input launch: read x and x_hat, write a and b.  The SGA step is the model of
tests/test_hip_fullsize.py::test_sga_step_at_tecnick_shape (two_layer_syn2, hidden 24, one 1200 x 1200 image), fetch=False."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as graft  # noqa: E402

graft.load_package()
from shallow_ntc_amd import ops  # noqa: E402
from shallow_ntc_amd.common import data_lib  # noqa: E402
from shallow_ntc_amd.mshyper import configs  # noqa: E402
from shallow_ntc_amd.mshyper.models import Model  # noqa: E402


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


def with_traffic(ms, nbytes):
    return dict(ms=ms, bytes=int(nbytes), gb_per_s=round(nbytes / (ms * 1e-3) / 1e9, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "msssim_grad.json"))
    ap.add_argument("--reps", type=int, default=25)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0), kernel="fused: one sntc_ssim_scale_grad launch per scale, 16 x 16 tile of g per workgroup",
               timer=f"median of {args.reps} after warm-up; HIP events on the launch stream", shapes={}, sga_step={})
    lam = 50.0
    for n, h, w in ((5, 1200, 1200), (18, 512, 768), (1, 512, 768)):
        x = torch.from_numpy(data_lib.normalize_image(data_lib.synthetic_images(n, h, w, seed=11))).to(dev)
        x_hat = (x + 0.03 * torch.randn_like(x)).contiguous()
        a, b, _ = ops.msssim_inputs(x, x_hat)
        r = dict(forward_ms=gpu_median_ms(lambda: ops.image_quality_launch(a, b, 255.0), args.reps),
                 value_and_gradient_ms=gpu_median_ms(lambda: ops.msssim_distortion_grad(x, x_hat, lam), args.reps),
                 mse_distortion_grad_ms=gpu_median_ms(lambda: ops.distortion_grad(x, x_hat, 1.0), args.reps))
        r["value_and_gradient_over_forward"] = round(r["value_and_gradient_ms"] / r["forward_ms"], 3)
        r["inputs"] = with_traffic(gpu_median_ms(lambda: ops.msssim_inputs(x, x_hat), args.reps), 4 * 4 * x.numel())
        sizes = ops.msssim_scale_sizes(h, w)
        pyr = [(a, b)]
        sums = torch.empty((len(sizes), 2, n, 3), dtype=torch.float64, device=dev)
        counts = []
        for k in range(len(sizes)):
            if k:
                pyr.append((ops._avgpool2(pyr[-1][0]), ops._avgpool2(pyr[-1][1])))
            counts.append(ops._ssim_scale(pyr[k][0], pyr[k][1], 255.0, sums[k]))
        r["finish_ms"] = gpu_median_ms(lambda: ops.msssim_finish(sums, counts, len(sizes) == 1, -lam / n), args.reps)
        _, coef = ops.msssim_finish(sums, counts, len(sizes) == 1, -lam / n)
        g, per_scale = None, {}
        for k in range(len(sizes) - 1, -1, -1):
            pa, pb = pyr[k]
            gc, last = g, k == len(sizes) - 1
            ms = gpu_median_ms(lambda: ops.ssim_scale_grad(pa, pb, coef[k], last, gc), args.reps)
            per_scale[f"scale{k}_{sizes[k][0]}x{sizes[k][1]}"] = with_traffic(ms, 4 * (3 * pa.numel() + (0 if gc is None else gc.numel())))
            g = ops.ssim_scale_grad(pa, pb, coef[k], last, gc)
        r["ssim_scale_grad"] = per_scale
        gc = torch.randn((n, (h + 1) // 2, (w + 1) // 2, 3), device=dev)
        r["avgpool2_symmetric_grad"] = with_traffic(gpu_median_ms(lambda: ops.avgpool2_symmetric_grad(gc, h, w), args.reps),
                                                    4 * (gc.numel() + n * h * w * 3))
        out["shapes"][f"{n}x{h}x{w}x3"] = r
        print(n, h, w, r, flush=True)
    x = torch.from_numpy(data_lib.normalize_image(data_lib.synthetic_images(1, 1200, 1200, seed=12))).to(dev)
    for distortion, rd_lambda in (("mse", 0.02), ("ms_ssim", 50.0)):
        cfg = {**configs.two_layer_syn2(rd_lambda=rd_lambda, hidden_channels=24), **configs.itinf()}
        model = Model(device=dev, distortion=distortion, **cfg)
        model.initialize_itinf(x)
        out["sga_step"][distortion] = gpu_median_ms(lambda: model.itinf_train_step(x, seed=1, fetch=False), args.reps)
        model.itinf_last_metrics()
    out["sga_step"]["ms_ssim_over_mse"] = round(out["sga_step"]["ms_ssim"] / out["sga_step"]["mse"], 3)
    print(out["sga_step"], flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
