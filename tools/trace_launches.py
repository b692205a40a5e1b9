#!/usr/bin/env python3
"""Per-launch durations of the decode's kernels (gather GEMM and its split-K finish, synthesis, dequantisation, output layer,
zeroing) in a rocprofv3 kernel trace, grouped by (kernel, workgroups):

    python tools/trace_launches.py <..._kernel_trace.csv>

A kernel name alone mixes the launches of different layers; its block count tells them apart."""
import csv, sys, collections, re
f=sys.argv[1]
rows=list(csv.DictReader(open(f)))
k=collections.defaultdict(list)
for r in rows:
    name=r["Kernel_Name"]
    if not any(w in name for w in ("gg_kernel", "syn_kernel", "gg_reduce_kernel", "dequant_kernel", "two_layer_tail_kernel", "zero_words_kernel")): continue
    short=re.sub(r"\(sntc.*","",name.replace("void sntc::",""))
    grid=int(r["Grid_Size_X"] if "Grid_Size_X" in r else r["Grid_Size"])//int(r.get("Workgroup_Size_X") or r.get("Workgroup_Size"))
    k[(short,grid)].append((int(r["End_Timestamp"])-int(r["Start_Timestamp"]))/1e3)
for key,v in sorted(k.items(), key=lambda kv:-sum(kv[1])):
    v2=sorted(v)
    print(f"{key[0]:70s} blocks={key[1]:5d} calls={len(v):3d} median {v2[len(v2)//2]:8.1f} us  min {v2[0]:8.1f}  total {sum(v)/1e3:7.2f} ms")
