#!/usr/bin/env python3
"""Mean of every counter per (kernel, workgroups) over the counter_collection CSVs of the given rocprofv3 --pmc directories."""
import collections, csv, glob, re, sys
agg = collections.defaultdict(lambda: collections.defaultdict(list))
for d in sys.argv[1:]:
    for f in glob.glob(f"{d}/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"]
            if "gg_kernel" not in name:
                continue
            short = re.sub(r"\(sntc.*", "", name.replace("void sntc::", ""))
            try:
                grid = int(r.get("Grid_Size_X") or r["Grid_Size"]) // int(r.get("Workgroup_Size_X") or r["Workgroup_Size"])
            except Exception:
                grid = -1
            agg[(short, grid)][r["Counter_Name"]].append(float(r["Counter_Value"]))
for key, v in sorted(agg.items(), key=lambda kv: -sum(kv[1].get("SQ_BUSY_CYCLES", [0]))):
    m = {c: sum(x) / len(x) for c, x in v.items()}
    print(f"{key[0]:70s} blocks={key[1]:5d} n={max(len(x) for x in v.values()):3d} " + " ".join(f"{c}={val:.4g}" for c, val in sorted(m.items())))
