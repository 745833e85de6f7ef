"""Per-pass kernel times of atr_denoise from a kernel trace of tools/denoise_bench.py:
reads the trace's *_kernel_trace.csv, takes every run of one denoise_pack_kernel followed by its
denoise_pass_kernel launches, groups the runs by grid size and prints, per size, the median, min and max
duration in microseconds of the pack kernel and of each pass in launch order (pass p has spacing 2^p).

python tools/denoise_trace_summary.py TRACE_DIR [--skip N]   (N leading calls per size dropped as warm-up)"""
import argparse
import csv
import glob
import json
import os

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("dir")
ap.add_argument("--skip", type=int, default=2)
args = ap.parse_args()
rows = []
for path in glob.glob(os.path.join(args.dir, "**", "*kernel_trace.csv"), recursive=True):
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            if "denoise_" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"],
                             int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"])))
rows.sort()
calls, cur = {}, None
for t0, t1, name, grid in rows:
    if "denoise_pack_kernel" in name:
        cur = [t1 - t0]
        calls.setdefault(grid, []).append(cur)
    elif cur is not None:
        cur.append(t1 - t0)
res = {}
for grid, lst in sorted(calls.items()):
    lst = [c for c in lst[args.skip:] if len(c) == len(lst[-1])]
    a = np.array(lst, np.float64) / 1000.0
    names = ["pack"] + [f"pass{p}" for p in range(a.shape[1] - 1)]
    res[f"pack_grid_{grid}"] = {"calls": len(lst), **{n: {"median": round(float(np.median(a[:, k])), 1),
                                                          "min": round(float(a[:, k].min()), 1),
                                                          "max": round(float(a[:, k].max()), 1)}
                                                      for k, n in enumerate(names)},
                                "sum_of_medians": round(float(np.median(a, axis=0).sum()), 1)}
print(json.dumps(res))
