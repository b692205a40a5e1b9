#!/usr/bin/env python3
"""Rate-distortion optimised quantisation (csrc/rdoq.hip, DESIGN.md 4.7 "RDOQ"): what the kernel costs beside the launches it
stands between, and what ``compress(x, rdoq=...)`` does to bits, SSE and J on the fixture models.

    python tools/profile_rdoq.py [--out profiles/rdoq.json] [--reps 25]

Latents of a 24 x 512 x 768 batch at C = 320 ([24, 32, 48, 320] floats around mu, spread as their tables; scale indexes over
all 64 tables).  Recorded:
  * ``sntc_rdoq_symbols`` (every image enabled, both values of ``flags``; every image disabled) and ``sntc_rdoq_map_symbols`` next
    to ``sntc_step_symbols`` + ``sntc_rans_cost``, the two launches whose work it combines, and against its traffic, 18 bytes per
    element (y, mu, id in; symbol, id out) at the 6.3 TB/s a streaming read achieves;
  * per image of the fixture models (random weights with the scale biases spread: NO rate-distortion gain of a trained model is
    claimed or can be read off these), the report of ``compress(x, rdoq=...)`` at several steps and strengths: delta bits, delta
    SSE, delta J of the RDOQ candidate against the plain one, and whether the guard used it.
Kernel figures: warm-up, then the median of ``reps`` runs between two HIP events on the launch stream, the variants alternating
inside one loop (output allocations and the zeroing of the counter included).  No figure here is a gate."""
import argparse
import json
import statistics
import sys
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


def fixture_model(cfg, dev):
    model = Model(device=dev, **cfg)
    wts = dict(model.get_weights())
    b = wts["hyper_synthesis/layer_2/bias"].copy()
    c = b.size // 2
    b[c:] = np.random.default_rng(0).uniform(-1.0, 2.5, size=c)          # spread the scale indexes (random weights leave them at the floor)
    wts["hyper_synthesis/layer_2/bias"] = b.astype(np.float32)
    model.set_weights(wts)
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rdoq.json"))
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--images", type=int, default=24)
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
    _, inv, sh = ec.step_tensors([0] * n, dev)
    lut = ec.step_lut(dev)
    kmap = torch.from_numpy(rng.integers(-8, 9, size=(n, h, w)).astype(np.int8)).to(dev)
    weight = torch.from_numpy((rng.uniform(0.05, 4.0, c) * 65536).astype(np.float32)).to(dev)
    on, off = torch.ones(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)

    def plain():
        sym, tid = ops.step_symbols(yd, hd, base, inv, sh)
        return sym, tid, ec.rans_cost(sym, tid, dt)

    sym0, tid0, cost0 = plain()
    got = ops.rdoq_symbols(yd, hd, base, inv, sh, weight, off, 1, dt)
    assert torch.equal(got[0], sym0) and torch.equal(got[1], tid0)
    sym1, tid1, changed = ops.rdoq_symbols(yd, hd, base, inv, sh, weight, on, 1, dt)
    cost1 = ec.rans_cost(sym1, tid1, dt)
    assert bool((cost1 <= cost0).all())
    elements = int(yd.numel())
    fns = {"rdoq_symbols_flags1_ms": lambda: ops.rdoq_symbols(yd, hd, base, inv, sh, weight, on, 1, dt),
           "rdoq_symbols_flags0_ms": lambda: ops.rdoq_symbols(yd, hd, base, inv, sh, weight, on, 0, dt),
           "rdoq_symbols_disabled_ms": lambda: ops.rdoq_symbols(yd, hd, base, inv, sh, weight, off, 1, dt),
           "rdoq_map_symbols_flags1_ms": lambda: ops.rdoq_map_symbols(yd, hd, base, kmap, lut, weight, on, 1, dt),
           "step_symbols_ms": lambda: ops.step_symbols(yd, hd, base, inv, sh),
           "rans_cost_ms": lambda: ec.rans_cost(sym0, tid0, dt),
           "step_symbols_plus_rans_cost_ms": plain}
    out = dict(device=torch.cuda.get_device_name(0), latents=[n, h, w, c], elements=elements,
               timer=f"median of {args.reps} after warm-up, variants alternating; HIP events on the launch stream (output allocations "
                     "and the zeroing of the counter included)",
               changed_share=round(float(changed.sum().item()) / elements, 4),
               bits_saved_share=round(1.0 - float(cost1.sum().item()) / float(cost0.sum().item()), 4))
    out["launches"] = gpu_medians_ms(fns, args.reps)
    t = out["launches"]["rdoq_symbols_flags1_ms"]
    traffic = 18 * elements
    out["rdoq_traffic_bytes"] = traffic
    out["rdoq_traffic_floor_ms"] = round(traffic / (STREAM_TBS * 1e12) * 1e3, 4)
    out["rdoq_tbs"] = round(traffic / (t * 1e-3) / 1e12, 3)
    out["rdoq_over_symbols_plus_cost"] = round(t / out["launches"]["step_symbols_plus_rans_cost_ms"], 2)
    print(json.dumps(out, indent=1), flush=True)

    rows = []
    for name, cfg in (("two_layer_syn", configs.two_layer_syn(rd_lambda=0.02)), ("jpegl", configs.jpegl(rd_lambda=0.02))):
        model = fixture_model(cfg, dev)
        gains = model.latent_gains()
        x = torch.from_numpy(data_lib.normalize_image(data_lib.synthetic_images(4, 256, 384, seed=11))).to(dev)
        for step in (None, -8, 8):
            for strength in (1.0, 0.1, 0.01):
                model.compress(x, step=step, rdoq=dict(strength=strength))
                for i, r in enumerate(model.last_compress_report):
                    rows.append(dict(model=name, image=i, step=0 if step is None else step, strength=strength, rdoq_used=r["rdoq_used"],
                                     changed=r["changed"], delta_bits=round(r["bits_rdoq"] - r["bits_plain"], 2),
                                     delta_sse=r["sse_rdoq"] - r["sse_plain"], delta_J=r["J_rdoq"] - r["J_plain"]))
        out.setdefault("gains", {})[name] = dict(min=float(gains.min()), median=float(np.median(gains)), max=float(gains.max()))
    out["fixture_models"] = dict(note="random weights, scale biases spread: the path runs and this is what it does HERE; no rate-distortion "
                                      "gain of a trained model is claimed", images=[4, 256, 384], rows=rows)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
