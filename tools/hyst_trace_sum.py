#!/usr/bin/env python3
"""The hysteresis chain's share of a step, from a rocprofv3 kernel-trace CSV of bench.py: over the second half of the front
kernel's launches (the clocks are up, the adaptive schedule has settled), per step -- one front-kernel launch -- the summed
duration of the k_hyst launches, how many there were, and the duration of the longest one (launch 0 of a chain on dense
content); the front kernel beside them.

  python tools/hyst_trace_sum.py <kernel_trace.csv> [...]"""
import csv
import statistics
import sys

for path in sys.argv[1:]:
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    fronts = [r for r in rows if "hc::k_front" in r["Kernel_Name"]]
    half = fronts[len(fronts) // 2:]
    t0 = int(half[0]["Start_Timestamp"])
    hyst = [r for r in rows if "hc::k_hyst" in r["Kernel_Name"] and int(r["Start_Timestamp"]) >= t0]
    steps = len(half)
    print(f"{path}: {steps} steps")
    print(f"  front kernel: median {statistics.median(dur(r) for r in half):.1f} us")
    print(f"  k_hyst: {len(hyst) / steps:.1f} launches per step, summed duration {sum(dur(r) for r in hyst) / steps:.1f} us per step, "
          f"launches over 100 us: {sum(dur(r) > 100 for r in hyst) / steps:.2f} per step, median of those {statistics.median([dur(r) for r in hyst if dur(r) > 100] or [0]):.1f} us")
