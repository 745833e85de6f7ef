"""Kernel times of atr_accumulate from a kernel trace of tools/accumulate_bench.py: reads
the trace's *_kernel_trace.csv, takes every accumulate_kernel dispatch, groups them by grid size and prints,
per size, the count and the median, min and max duration in microseconds (the camera at rest and the
orbit step together; the one dispatch per size that starts the history is dropped with the warm-up).

python tools/accumulate_trace_summary.py TRACE_DIR [--skip N]   (N leading dispatches per size dropped)"""
import argparse
import csv
import glob
import json
import os

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("dir")
ap.add_argument("--skip", type=int, default=5)
args = ap.parse_args()
rows = []
for path in glob.glob(os.path.join(args.dir, "**", "*kernel_trace.csv"), recursive=True):
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            if "accumulate_kernel" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]),
                             int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"])))
rows.sort()
by = {}
for t0, t1, grid in rows:
    by.setdefault(grid, []).append((t1 - t0) / 1000.0)
stat = lambda a: {"n": len(a), "median": round(float(np.median(a)), 1), "min": round(float(np.min(a)), 1),  # noqa: E731
                  "max": round(float(np.max(a)), 1)}
res = {}
for grid, lst in sorted(by.items()):
    lst = lst[args.skip:]
    res[f"grid_{grid}"] = stat(lst)
print(json.dumps(res))
