#!/usr/bin/env python3
"""Per-content duration of the front kernel from a rocprofv3 kernel trace of the default benchmark
(rocprofv3 --kernel-trace --stats --output-format csv -- python3 bench.py --gpus 1 --steps 100 --warmup 10).
Usage: tools/front_per_content.py <..._kernel_trace.csv> <label> [timed steps, default 100]

The benchmark launches one front kernel per step and its timed steps are its last ones, beginning with the rotation's
first content: the last N k_front8 launches in start order are the timed steps, and launch j of them processed content
j % 4 (0 natural, 1 natural-B, 2 noise, 3 blend).  Printed per content: launches, median, minimum, maximum (us)."""
import csv
import statistics
import sys

rows = []
for r in csv.DictReader(open(sys.argv[1])):
    if "k_front8<" in r["Kernel_Name"] or "k_front8I" in r["Kernel_Name"]:
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
rows.sort()
N = int(sys.argv[3]) if len(sys.argv) > 3 else 100
timed = rows[-N:]
off = 0
print("build,launch_mod_4,launches,median_us,min_us,max_us")
for k in range(4):
    t = [d / 1e3 for j, (_, d) in enumerate(timed) if (off + j) % 4 == k]
    print("%s,%d,%d,%.1f,%.1f,%.1f" % (sys.argv[2], k, len(t), statistics.median(t), min(t), max(t)))
print("# front launches in the trace:", len(rows))
