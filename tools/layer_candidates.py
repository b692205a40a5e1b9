#!/usr/bin/env python3
"""Every (tile variant, schedule, forced stream-K unit order) candidate of the last hyper-synthesis layer (3x3 / 1, 480 -> 640),
as the decoder's 320-column launch and as the whole layer, at the two Kodak batch shapes: device idle, HIP events, three
interleaved rounds of 20 launches per candidate, sorted by the median round (profiles/hs3_candidates.txt).  Every candidate is
compared bit for bit with the cost model's launch before it is timed.

    python tools/layer_candidates.py [out.json]
"""
import sys, json
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch
import __graft_entry__ as g
g.load_package()
from shallow_ntc_amd import ops

dev = "cuda:0"
gen = torch.Generator(device=dev); gen.manual_seed(5)
rows = []

def clock(fn, reps=20):
    for _ in range(3): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / reps

def measure(name, plan, target, shapes):
    for (n, h, w) in shapes:
        x = torch.randn((n, h, w, plan.cin), device=dev, generator=gen)
        ref = target(x).clone()
        model = target.launch_info(n, h, w) + (target.launch_order(n, h, w),)
        cands = []
        for v, sk in target.candidates(n, h, w):
            for colm in ((None, False, True) if sk else (None,)):
                cands.append((v, sk, colm))
        times = {c: [] for c in cands}
        info = {}
        for rnd in range(3):
            for c in cands:
                v, sk, colm = c
                plan.set_stream_k(True, colm=colm)
                target.set_choice(n, h, w, v, sk)
                info[c] = target.launch_info(n, h, w) + (target.launch_order(n, h, w),)
                if rnd == 0:
                    assert torch.equal(target(x), ref), c
                times[c].append(clock(lambda: target(x)))
        plan.set_stream_k(True); target.drop_choice(n, h, w)
        fl = target.flops(n, h, w)
        print(f"== {name} n={n} h={h} w={w}  cost model picks variant {model[0]} blocks {model[1]} colm {model[2]}")
        for c in sorted(cands, key=lambda c: sorted(times[c])[1]):
            t = sorted(times[c])
            print(f"  v={c[0]:2d} sk={c[1]} colm_forced={str(c[2]):5s} -> launched v={info[c][0]:2d} blocks={info[c][1]:4d} colm={int(info[c][2])}  "
                  f"median {t[1]*1e3:7.1f} us  (min {t[0]*1e3:7.1f} max {t[2]*1e3:7.1f})  {fl/t[1]/1e9:6.1f} TFLOP/s")
            rows.append(dict(layer=name, n=n, h=h, w=w, variant=c[0], sk=c[1], colm_forced=c[2], blocks=info[c][1], colm=bool(info[c][2]), us=[round(v*1e3, 2) for v in t]))
        sys.stdout.flush()

hs3 = ops.ConvPlan("convT", torch.randn((3, 3, 640, 480), device=dev, generator=gen) * 0.02, torch.randn((640,), device=dev, generator=gen), 1)
measure("HS3 480->320 cols (3x3/1)", hs3, hs3.columns(320), [(18, 32, 48), (6, 48, 32)])
measure("HS3 480->640 whole (3x3/1)", hs3, hs3, [(18, 32, 48), (6, 48, 32)])
ops.check_conv_status()
if len(sys.argv) > 1:
    Path(sys.argv[1]).write_text(json.dumps(rows))
