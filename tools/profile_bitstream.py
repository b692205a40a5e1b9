#!/usr/bin/env python3
"""Time the rANS stages of Model.compress / decompress (HIP events on the launch stream) and report the
real-vs-estimated rate.  python tools/profile_bitstream.py [--batch 18] [--hw 512 768] [--segments 2]

    python tools/profile_bitstream.py --step-map profiles/step_map.json [--reps 25]      (at least 25 repetitions)
measures region-of-interest coding instead (csrc/quant_step.hip, DESIGN.md 4.7 "variable rate") and writes the JSON:
  * ``sntc_step_map_ladder_cost`` at 16 candidates against ``sntc_step_ladder_cost`` at the same 16, on the latents of an
    18 x 512 x 768 batch at C = 320 (those of tools/profile_quant_step.py), with offsets 0 on a centred rectangle and +12 around
    it, and with offsets all 0 (the same integers as the uniform launch: asserted);
  * ``Model.compress(x, target_bpp=..., step_offsets=...)`` against ``Model.compress(x, target_bpp=...)`` (host wall clock).
Launches: warm-up, then the median of ``reps`` runs between two HIP events, the variants alternating inside one loop."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

import __graft_entry__ as graft

graft.load_package()
from shallow_ntc_amd import entropy_coding as ec
from shallow_ntc_amd import ops
from shallow_ntc_amd.common import data_lib
from shallow_ntc_amd.mshyper import configs
from shallow_ntc_amd.mshyper.models import Model

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=18)
ap.add_argument("--hw", type=int, nargs=2, default=[512, 768])
ap.add_argument("--segments", type=int, default=2)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--step-map", default=None, metavar="JSON", help="measure the step-map ladder and rate control instead; write here")
args = ap.parse_args()


def profile_step_map(out_path, reps):
    from profile_quant_step import gpu_medians_ms, wall_medians_ms
    dev = torch.device("cuda:0")
    n, h, w, c = 18, 32, 48, 320
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
    tensors = ec.step_tensors(ladder, dev)
    lut, bases_d = ec.step_lut(dev), torch.tensor(ladder, dtype=torch.int32).to(dev)
    mask = np.zeros((n, 512, 768), np.bool_)
    mask[:, 128:384, 192:576] = True
    roi = ec.roi_offsets(mask, 16, inside=0, outside=12, grow=1)
    offs = {"roi": torch.from_numpy(roi).to(dev), "zero": torch.zeros((n, h, w), dtype=torch.int8, device=dev)}
    uniform = ec.step_ladder_cost(yd, hd, base, ladder, dt, tensors)
    assert torch.equal(ec.step_map_ladder_cost(yd, hd, base, offs["zero"], ladder, dt, lut, bases_d), uniform)
    fns = {"uniform_ladder_k16_ms": lambda: ec.step_ladder_cost(yd, hd, base, ladder, dt, tensors)}
    for name, o in offs.items():
        fns[f"map_ladder_k16_{name}_offsets_ms"] = lambda o=o: ec.step_map_ladder_cost(yd, hd, base, o, ladder, dt, lut, bases_d)
    out = dict(device=torch.cuda.get_device_name(0), latents=[n, h, w, c], elements=int(yd.numel()), ladder=ladder,
               roi_offsets=dict(inside=0, outside=12, grow=1, rectangle_pixels=[128, 384, 192, 576], runs_per_image=int(ec.count_runs(roi)[0])),
               timer=f"median of {reps} after warm-up, variants alternating; launches: HIP events on the launch stream (output "
                     "allocations and the zeroing of the sums included; steps / bases / tables uploaded before); compress: host wall "
                     "clock around a synchronised call")
    out["launches"] = gpu_medians_ms(fns, reps)
    out["launches_repeat"] = gpu_medians_ms(fns, reps, warmup=0)             # the same loop again: the run-to-run spread
    out["map_over_uniform"] = {k: round(v / out["launches"]["uniform_ladder_k16_ms"], 3) for k, v in out["launches"].items() if k.startswith("map")}
    print(json.dumps(out, indent=1), flush=True)

    model = Model(device=dev, **configs.two_layer_syn(rd_lambda=0.02))
    wts = dict(model.get_weights())
    b = wts["hyper_synthesis/layer_2/bias"].copy()
    b[c:] = np.random.default_rng(0).uniform(-1.0, 2.5, size=c)          # spread the scale indexes (random weights leave them at the floor)
    wts["hyper_synthesis/layer_2/bias"] = b.astype(np.float32)
    model.set_weights(wts)
    x = torch.from_numpy(data_lib.normalize_image(data_lib.synthetic_images(n, 512, 768, seed=11))).to(dev)
    roi = ec.roi_offsets(mask, 16, inside=0, outside=12, grow=1, latent_hw=model.step_offsets_shape(512, 768))
    codec = model._get_codec()
    lat = model.infer_latent_rvs(x)
    cz, cy = codec.ladder_cost(lat.uq[0].loc, lat.uq[1].loc, (512, 768), [0, 3])
    bits = (cz[:, None] + cy).cpu().numpy() / 65536.0 + codec.flushed_bits(512, 768)
    target = float(bits[:, 1].max() + 1.0) / (512 * 768)               # every image fits at uniform k = 3
    plain = model.compress(x, target_bpp=target)
    plain_steps = [q["step_chosen"] for q in model.last_compress_report]
    blob = model.compress(x, target_bpp=target, step_offsets=roi)
    rep = model.last_compress_report
    assert tuple(model.decompress(blob).shape) == (n, 512, 768, 3)
    r = dict(images=[n, 512, 768], target_bpp=round(target, 5), uniform_bytes=len(plain), uniform_steps=plain_steps, roi_bytes=len(blob),
             roi_version=blob[4], roi_bases=[q["step_chosen"] for q in rep], roi_met=[q["met"] for q in rep], map_bits=rep[0]["map_bits"])
    r.update(wall_medians_ms({"compress_target_bpp_ms": lambda: model.compress(x, target_bpp=target),
                              "compress_target_bpp_offsets_ms": lambda: model.compress(x, target_bpp=target, step_offsets=roi)},
                             max(8, reps // 3)))
    out["compress"] = r
    print(json.dumps(r, indent=1), flush=True)
    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    Path(out_path).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", out_path)


if args.step_map:
    profile_step_map(args.step_map, max(args.reps, 25))
    sys.exit(0)
ec.ELEMS_PER_SEGMENT = -(-(args.hw[0] // 16) * (args.hw[1] // 16) * 320 // args.segments)
dev = torch.device("cuda:0")
model = Model(device=dev, **configs.CONFIGS["two_layer_syn"]())
n, (h, w) = args.batch, args.hw
x = data_lib.synthetic_images(n, h, w, seed=1234) if hasattr(data_lib, "synthetic_images") else None
if x is None:
    x = np.random.default_rng(1234).integers(0, 256, (n, h, w, 3)).astype(np.uint8)
codec = model._get_codec()


def timed(fn):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), out


with torch.cuda.device(dev):
    xf = model._as_device_images(x)
    lat = model.infer_latent_rvs(xf)
    z, y = lat.uq[0].loc, lat.uq[1].loc
    zi = ec.round_to_int(z)
    hyper = model._hyper_synthesis(ec.int_to_float(zi))
    _, bits_y, sym = ops.entropy_scale_normal(y, hyper, want_symbols=True)
    ztid, ytid = ec.channel_table_ids(z.shape, dev), ec.scale_table_ids(hyper)
    t_ze, (zp, zl) = timed(lambda: ec.rans_encode(zi, ztid, codec.z_tables, args.segments))
    t_ye, (yp, yl) = timed(lambda: ec.rans_encode(sym, ytid, codec.y_tables, args.segments))
    t_zd, zi2 = timed(lambda: ec.rans_decode(zp, zl, ztid, tuple(z.shape), codec.z_tables, args.segments))
    t_yd, sy2 = timed(lambda: ec.rans_decode(yp, yl, ytid, tuple(y.shape), codec.y_tables, args.segments))
    assert torch.equal(zi2, zi) and torch.equal(sy2, sym)
    blob = model.compress(x)
    px = model.decompress(blob)
    m = model.evaluate_batched(x) if hasattr(model, "evaluate_batched") else None
mpx = n * h * w / 1e6
print(f"segments {args.segments}: streams z {len(zl)} y {len(yl)}; encode z {t_ze:.3f} ms y {t_ye:.3f} ms (incl. length readback + compaction); "
      f"decode z {t_zd:.3f} ms y {t_yd:.3f} ms for {mpx:.2f} Mpixel")
print(f"bitstream {8 * len(blob) / (n * h * w):.4f} bpp real; y payload {16 * int(yl.sum()) / (n * h * w):.4f} bpp vs estimate "
      f"{float(bits_y.sum()) / (n * h * w):.4f} bpp")
