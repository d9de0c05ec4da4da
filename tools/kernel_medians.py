#!/usr/bin/env python3
"""Per-kernel launch times of one `rocprofv3 --kernel-trace --output-format csv` run: launches, median, min, mean, max in us, kernels
by total time.  The median and the min-max range are what two trees are compared by (an average carries the warm-up's first launches).
   python tools/kernel_medians.py <label> <dir with *kernel_trace.csv> [rows]"""
import csv
import glob
import os
import sys

import numpy as np


def main():
    label, root = sys.argv[1], sys.argv[2]
    rows = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    files = glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no *kernel_trace.csv under {root}")
    dur = {}
    for r in csv.DictReader(open(max(files, key=os.path.getsize))):
        dur.setdefault(r["Kernel_Name"].split("(")[0], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print(f"== {label}: per-kernel launch time in us (rocprofv3 --kernel-trace), kernels by total time")
    for name, d in sorted(dur.items(), key=lambda kv: -sum(kv[1]))[:rows]:
        d = np.asarray(d)
        print("%-7s %-48s launches %4d median %8.2f min %8.2f mean %8.2f max %8.2f" % (label, name[:48], d.size, np.median(d), d.min(), d.mean(), d.max()))


if __name__ == "__main__":
    main()
