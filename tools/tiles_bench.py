#!/usr/bin/env python3
"""Tiled files (csrc/tiles.hip, wire format 9, DESIGN.md 4.7 "tiled files"): what the two pixel-end kernels take next to a plain
device copy, what tiling costs in the file, and what a region decode and a full tiled decode take next to the untiled decode.

    timeout 900 python tools/tiles_bench.py [--out profiles/tiles.json] [--reps 15] [--side 4096]

Needs the GPU (no fallback).  Recorded:
  1. ``ops.tiles_extract`` (one launch per shape class) and ``sntc_tiles_assemble`` on one side x side picture at tile 512,
     overlap 16, next to ``Tensor.copy_`` of the same OUTPUT bytes, timed in the same process: median between two HIP events on
     the launch stream, the four callables alternating inside every repetition, after 5 warm-up rounds.  GB/s = output bytes over
     time for every row, so the ratio to the copy reads directly (a copy reads what it writes; assemble reads 1 .. 4 tile values
     per output value, extract reads what it writes).  Reported, not asserted.
  2. the rate price of tiling on the Kodak-shaped synthetic set (18 x 512 x 768 + 6 x 768 x 512): bytes of
     ``compress(x, tile=256, overlap=0 | 16)`` against ``compress(x)``, PSNR of each decode alongside.
  3. ``decompress(blob, region=...)`` of a 512 x 512 window of the side x side tiled file -- one that meets four tiles and one,
     aligned to the tile grid, that meets nine -- against the full ``decompress`` of that file.
  4. that full tiled decode against ``decompress`` of the UNTILED file of the same picture: the untiled path is the code of the
     parent commit, unchanged (a file without tiles never reaches the tiled branch), so this is the parent's decode in the same
     process.  Calls: host wall clock around a call that ends in its own synchronising read-back, variants alternating, median /
     min / max after 3 warm-up rounds.
The model is two_layer_syn with seeded random weights and spread scale biases on synthetic images: times and byte RATIOS say what
the path costs on this model; nothing is claimed for trained weights, and the PSNR of random weights is only a consistency
figure (tiling must not move it much)."""
import argparse
import ctypes as C
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
from profile_transcode import psnr, wall_stats_ms  # noqa: E402
from shallow_ntc_amd import _capi as capi  # noqa: E402
from shallow_ntc_amd import ops, tiling  # noqa: E402
from shallow_ntc_amd.common import data_lib  # noqa: E402
from shallow_ntc_amd.mshyper import configs  # noqa: E402
from shallow_ntc_amd.mshyper.models import Model  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tiles.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--side", type=int, default=4096)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tiles_bench: no GPU; nothing is measured without one")
    dev = torch.device("cuda:0")
    model = Model(device=dev, **configs.two_layer_syn(rd_lambda=0.02))
    wts = dict(model.get_weights())
    b = wts["hyper_synthesis/layer_2/bias"].copy()
    b[320:] = np.random.default_rng(0).uniform(-1.0, 2.5, size=320)      # spread the scale indexes (random weights leave them at the floor)
    wts["hyper_synthesis/layer_2/bias"] = b.astype(np.float32)
    model.set_weights(wts)
    S, T, O = args.side, 512, 16
    out = dict(device=torch.cuda.get_device_name(0), side=S, tile=T, overlap=O, reps=args.reps,
               model="two_layer_syn, seeded random weights with spread scale biases, synthetic images")

    # 1. the kernels next to a plain device copy of their output bytes
    big = torch.from_numpy(data_lib.normalize_image(data_lib.synthetic_images(1, S, S, seed=77))).to(dev)
    g, plan, _ = tiling.tile_plan(1, S, S, T, O)
    rects = [[(i, g["rows"][r][2], g["cols"][c][2]) for i, r, c in bl["tiles"]] for bl in plan]
    extract_bytes = 4 * 3 * sum(bl["th"] * bl["tw"] * len(bl["tiles"]) for bl in plan)
    src_f, dst_f = (torch.empty(extract_bytes // 4, dtype=torch.float32, device=dev) for _ in range(2))
    src_f.normal_()
    rng = np.random.default_rng(3)
    tiles = [torch.from_numpy(rng.integers(0, 256, (y1 - y0, x1 - x0, 3), dtype=np.uint8)).to(dev)
             for _, _, y0, y1 in g["rows"] for _, _, x0, x1 in g["cols"]]
    table = torch.from_numpy(np.array([t.data_ptr() for t in tiles], np.int64)).to(dev)
    px = torch.empty((1, S, S, 3), dtype=torch.uint8, device=dev)
    missing = torch.empty((1,), dtype=torch.int32, device=dev)
    src_b = torch.randint(0, 256, (S * S * 3,), dtype=torch.uint8, device=dev)
    dst_b = torch.empty_like(src_b)
    assemble = lambda: capi.call("sntc_tiles_assemble", C.c_void_p(table.data_ptr()), 1, S, S, 3, T, O, 0, 0, S, S,
                                 C.c_void_p(px.data_ptr()), C.c_void_p(missing.data_ptr()), ops._stream())
    k = gpu_medians_ms({"extract_ms": lambda: [ops.tiles_extract(big, r, bl["th"], bl["tw"]) for r, bl in zip(rects, plan)],
                        "copy_extract_bytes_ms": lambda: dst_f.copy_(src_f),
                        "assemble_ms": assemble,
                        "copy_assemble_bytes_ms": lambda: dst_b.copy_(src_b)}, max(25, args.reps))
    assert int(missing.item()) == 0
    gbs = lambda nbytes, ms: round(nbytes / (ms * 1e-3) / 1e9, 1)
    out["kernels"] = dict(**k, extract_output_bytes=extract_bytes, assemble_output_bytes=int(px.numel()), extract_launches=len(plan),
                          extract_gbs=gbs(extract_bytes, k["extract_ms"]), copy_extract_gbs=gbs(extract_bytes, k["copy_extract_bytes_ms"]),
                          assemble_gbs=gbs(px.numel(), k["assemble_ms"]), copy_assemble_gbs=gbs(px.numel(), k["copy_assemble_bytes_ms"]),
                          extract_over_copy=round(k["extract_ms"] / k["copy_extract_bytes_ms"], 2),
                          assemble_over_copy=round(k["assemble_ms"] / k["copy_assemble_bytes_ms"], 2),
                          note="GB/s = OUTPUT bytes over the median time; extract includes its output allocations and one launch per "
                               "shape class, assemble the kernel that zeroes its counter; ratios are time over the copy's time")
    print(json.dumps(out["kernels"], indent=1), flush=True)
    del src_f, dst_f, src_b, dst_b, tiles, table, px

    # 2. the rate price of tiling, Kodak-shaped synthetic set
    xs = [torch.from_numpy(data_lib.normalize_image(data_lib.synthetic_images(n, h, w, seed=11 + n))).to(dev)
          for n, h, w in ((18, 512, 768), (6, 768, 512))]
    pixels = sum(int(x.shape[0] * x.shape[1] * x.shape[2]) for x in xs)
    rows = []
    for label, kw in (("untiled", {}), ("tile 256, overlap 0", dict(tile=256, overlap=0)), ("tile 256, overlap 16", dict(tile=256, overlap=16))):
        files = [model.compress(x, **kw) for x in xs]
        dec = model.decompress_many(files)
        nbytes = sum(len(f) for f in files)
        sse = sum(float(((p.double() - torch.round((x.double() + 0.5) * 255.0)) ** 2).sum().item()) for p, x in zip(dec, xs))
        rows.append(dict(file=label, bytes=nbytes, bpp=round(8.0 * nbytes / pixels, 4),
                         psnr_db=round(float(10.0 * np.log10(255.0 ** 2 * 3 * pixels / sse)), 3)))
    for r in rows[1:]:
        r["bytes_over_untiled"] = round(r["bytes"] / rows[0]["bytes"], 4)
    out["rate"] = rows
    print(json.dumps(rows, indent=1), flush=True)
    del xs

    # 3. + 4. region decode, full tiled decode, the untiled decode of the same picture
    def decode_part(x):
        side = int(x.shape[1])
        tiled = model.compress(x, tile=T, overlap=O)
        full = model.decompress(tiled)
        four, nine = (side // 2 + T // 2, side // 2 + T // 2, 512, 512), (side // 2, side // 2, 512, 512)
        reports = {}
        for name, win in (("window_4_tiles", four), ("window_9_tiles", nine)):
            got = model.decompress(tiled, region=win)
            assert torch.equal(got, full[:, win[0]:win[0] + win[2], win[1]:win[1] + win[3]])
            reports[name] = dict(region=list(win), **model.last_decompress_report)
        fns = {"region_4_tiles": lambda: model.decompress(tiled, region=four), "region_9_tiles": lambda: model.decompress(tiled, region=nine),
               "tiled_full": lambda: model.decompress(tiled)}
        part = dict(side=side, reports=reports, tiled_bytes=len(tiled), tiled_psnr_db=round(psnr(full, x), 3))
        try:                                            # a single image whose layers pass 2^31 bytes is refused untiled: recorded, not hidden
            plain = model.compress(x)
            part.update(untiled_bytes=len(plain), untiled_psnr_db=round(psnr(model.decompress(plain), x), 3))
            fns["untiled_full"] = lambda: model.decompress(plain)
        except (capi.SntcError, ValueError, RuntimeError) as e:
            part["untiled_refused"] = str(e)[:300]
        calls = wall_stats_ms(fns, args.reps)
        part["calls"] = calls
        med = lambda key: calls[key]["median_ms"]
        part.update(region_4_over_tiled_full=round(med("region_4_tiles") / med("tiled_full"), 3),
                    region_9_over_tiled_full=round(med("region_9_tiles") / med("tiled_full"), 3))
        if "untiled_full" in calls:
            part["tiled_over_untiled"] = round(med("tiled_full") / med("untiled_full"), 3)
        return part

    out["decode"] = [decode_part(big)]
    if "untiled_refused" in out["decode"][0] and S >= 2048:
        out["decode"].append(decode_part(big[:, :S // 2, :S // 2].contiguous()))
    out["decode_note"] = "untiled_full runs the parent commit's decode path unchanged; every call ends in its own read-back"
    print(json.dumps(out["decode"], indent=1), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
