#!/usr/bin/env python3
"""The SSIM / MS-SSIM forward (csrc/msssim.hip) of this tree against another build of the library, alternating in one process:

    python tools/profile_ssim_forward.py --parent-lib /path/to/parent/libsntc_hip.so [--out profiles/ssim_forward.json] [--reps 31]

``--parent-lib``: libsntc_hip.so built from the commit to compare with.  Both libraries are loaded side by side and run the launch
sequence of ``ops.image_quality_launch`` (pool + sntc_ssim_scale per scale, 5 scales) on the same device tensors, 1 x 512 x 768 x 3
and 18 x 512 x 768 x 3.  Per shape: warm-up of both, then ``reps`` rounds of parent, this tree, parent, ... each timed between two
HIP events on the launch stream (output allocations outside).  Written: both medians, the parent's run-to-run spread (min,
quartiles, max), whether this tree's median lies within it, and the largest relative difference of the sums (the two builds
differ by the forward's tile centring)."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as graft  # noqa: E402

graft.load_package()
from shallow_ntc_amd import _capi, ops  # noqa: E402
from shallow_ntc_amd.common import data_lib  # noqa: E402


def bind(path):
    lib = C.CDLL(str(path))
    for name in ("sntc_ssim_scale", "sntc_avgpool2_symmetric"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _capi.SIGNATURES[name]
    return lib


def forward(lib, pyramid, sums, stream):
    """pyramid: [(a_k, b_k)] preallocated per scale; scale 0 holds the images."""
    for k, (a, b) in enumerate(pyramid):
        n, h, w, c = a.shape
        if k > 0:
            pa, pb = pyramid[k - 1]
            for src, dst in ((pa, a), (pb, b)):
                rc = lib.sntc_avgpool2_symmetric(src.data_ptr(), n, src.shape[1], src.shape[2], c, dst.data_ptr(), stream)
                assert rc == 0, rc
        rc = lib.sntc_ssim_scale(a.data_ptr(), b.data_ptr(), n, h, w, c, 255.0, sums[k, 0].data_ptr(), sums[k, 1].data_ptr(), stream)
        assert rc == 0, rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ssim_forward.json"))
    ap.add_argument("--reps", type=int, default=31)
    args = ap.parse_args()
    assert args.reps >= 25
    dev = torch.device("cuda:0")
    libs = dict(parent=bind(args.parent_lib), this=bind(_capi.LIB_PATH))
    stream = torch.cuda.current_stream().cuda_stream
    out = dict(device=torch.cuda.get_device_name(0), what="launch sequence of ops.image_quality_launch: 8 pool + 5 sntc_ssim_scale launches",
               timer=f"warm-up, then {args.reps} alternating rounds; HIP events on the launch stream; milliseconds", shapes={})
    for n, h, w in ((1, 512, 768), (18, 512, 768)):
        x = torch.from_numpy(data_lib.normalize_image(data_lib.synthetic_images(n, h, w, seed=11))).to(dev)
        a, b, _ = ops.msssim_inputs(x, (x + 0.03 * torch.randn_like(x)).contiguous())
        sizes = ops.msssim_scale_sizes(h, w)
        pyramid = [(a, b)] + [tuple(torch.empty((n, sh, sw, 3), dtype=torch.float32, device=dev) for _ in range(2)) for sh, sw in sizes[1:]]
        sums = {k: torch.empty((len(sizes), 2, n, 3), dtype=torch.float64, device=dev) for k in libs}
        for _ in range(5):
            for k, lib in libs.items():
                forward(lib, pyramid, sums[k], stream)
        torch.cuda.synchronize()
        ts = {k: [] for k in libs}
        for _ in range(args.reps):
            for k, lib in libs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                forward(lib, pyramid, sums[k], stream)
                e1.record()
                e1.synchronize()
                ts[k].append(e0.elapsed_time(e1))
        qs = statistics.quantiles(ts["parent"], n=4)
        r = dict(parent_median=round(statistics.median(ts["parent"]), 4), this_median=round(statistics.median(ts["this"]), 4),
                 parent_spread=dict(min=round(min(ts["parent"]), 4), q1=round(qs[0], 4), q3=round(qs[2], 4), max=round(max(ts["parent"]), 4)),
                 this_spread=dict(min=round(min(ts["this"]), 4), max=round(max(ts["this"]), 4)))
        r["this_median_within_parent_spread"] = bool(r["parent_spread"]["min"] <= r["this_median"] <= r["parent_spread"]["max"])
        r["this_over_parent"] = round(r["this_median"] / r["parent_median"], 4)
        r["max_rel_diff_of_sums"] = float(((sums["this"] - sums["parent"]).abs() / sums["parent"].abs()).max())
        out["shapes"][f"{n}x{h}x{w}x3"] = r
        print(n, h, w, r, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
