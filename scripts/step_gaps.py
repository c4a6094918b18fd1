#!/usr/bin/env python3
"""One NN-graph step of a `rocprofv3 --kernel-trace --memory-copy-trace` run of bench.py as a list of device operations
(kernels and copies, in start order) with the idle time in front of each: python scripts/step_gaps.py DIR [LAPS]

DIR holds *_kernel_trace.csv and *_memory_copy_trace.csv; the step listed is the last one (it begins behind the
CSR kernels of the step before it and the copies that fetch their result).  LAPS: the stderr of an ISOCON_DEBUG=1 run of the same build; the
laps of its last call are appended.  profiles/step_gaps_*.txt are outputs of this script."""
import csv
import glob
import os
import re
import sys


def load(d):
    ops = []
    for f in glob.glob(os.path.join(d, "**", "*_kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = re.sub(r"\(anonymous namespace\)::|isocon::", "", r["Kernel_Name"])
            name = re.sub(r"\(.*", "", name)
            ops.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "kernel", name))
    for f in glob.glob(os.path.join(d, "**", "*_memory_copy_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            ops.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "copy", r["Direction"].replace("MEMORY_COPY_", "")))
    ops.sort()
    return ops


def main():
    ops = load(sys.argv[1])
    prof = [i for i, o in enumerate(ops) if o[3].startswith("k_qgram_profile4")]
    if not prof:
        raise SystemExit("no k_qgram_profile4 in the trace")
    # the step begins behind the CSR kernels of the step before it and the copies that fetch their result
    first = prof[-1]
    fin = [i for i in range(first) if ops[i][3].startswith("k_fin_")]
    first = fin[-1] + 1 if fin else 0
    while first < prof[-1] and (ops[first][3] == "DEVICE_TO_HOST" or "copyBuffer" in ops[first][3]):
        first += 1
    step = ops[first:]
    t0 = step[0][0]
    print("%-10s %-9s %-9s %-7s %s" % ("start us", "gap us", "run us", "kind", "operation"))
    busy = gaps = 0.0
    end = t0
    for s, e, kind, name in step:
        gap = max(0, s - end) / 1e3
        print("%10.1f %9.1f %9.1f %-7s %s" % ((s - t0) / 1e3, gap, (e - s) / 1e3, kind, name))
        gaps += gap
        busy += (e - s) / 1e3
        end = max(end, e)
    print("# %d operations (%d kernels, %d copies); first start to last end %.1f us; idle between operations %.1f us; sum of run times %.1f us"
          % (len(step), sum(o[2] == "kernel" for o in step), sum(o[2] == "copy" for o in step), (end - t0) / 1e3, gaps, busy))
    if len(sys.argv) > 2:
        lines = [ln.rstrip() for ln in open(sys.argv[2]) if ln.startswith("[isocon]")]
        starts = [i for i, ln in enumerate(lines) if "sync at entry" in ln]
        print("\n# ISOCON_DEBUG laps of the last call (host clock; the run waits for the device at entry and after setup)")
        for ln in lines[starts[-1] if starts else 0:]:
            print(ln)


if __name__ == "__main__":
    main()
