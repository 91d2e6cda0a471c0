"""Times hc_hough_lines_device over the C ABI (profiles/hough/README.md):

    python tools/hough_bench.py --content natural|noise [--frames N] [--threshold T] [--counts-only] [--rows A]

The point lists are hc_edge_points_device's of cv::Canny's maps (Mode O, canny_device, thresholds 50 / 150, aperture 3) of
bench.py's generators: 8 distinct 1920 x 1080 frames of synth.frames at bench.py's seeds, their lists repeated on the device to
`frames` lists; point_capacity = the largest count, so nothing is cut.  rho 1, theta pi / 180, [0, pi]: 180 angles, 6001 bins.
All launches of a call together are timed with events on the stream the context runs on (--counts-only: line_capacity 0, no
k_hough_rank); one measurement per process.  Prints one JSON line, and appends it to profiles/hough/hough_bench.jsonl with
--record: the times and the votes (points x angles) per second.  --rows A fixes the angles per workgroup of k_hough_vote
(HC_OPT_TEST_HOUGH_ROWS; the library caps it at the 6 rows of 6003 words that LDS holds) and is recorded as "rows_requested";
without it the library's plan chooses, and the line carries no row count: the library does not report its choice.
Per-kernel times come from running this tool under a kernel trace; --steps then sets the number of calls traced."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cudacam_amd import api, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--content", default="natural", choices=["natural", "noise"])
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--threshold", type=int, default=150)
    ap.add_argument("--max-lines", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=0, help="angles per workgroup of k_hough_vote (HC_OPT_TEST_HOUGH_ROWS); 0: the plan's rule")
    ap.add_argument("--counts-only", action="store_true", help="line_capacity 0: votes and peak counts, no ranking")
    ap.add_argument("--record", action="store_true", help="append the result to profiles/hough/hough_bench.jsonl")
    a = ap.parse_args()
    import torch
    w, h, n = 1920, 1080, a.frames
    rho, theta = 1.0, math.pi / 180
    src = synth.frames(a.content, w, h, 8, seed=synth.SEED0 + (9000 if a.content == "noise" else 0))
    s = torch.cuda.Stream()
    ctx = api.Context(w, h, 1, max(n, 8), api.MODE_O)
    maps = torch.from_numpy(ctx.canny(src, 50, 150)).cuda()
    pc8 = torch.zeros((8,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.edge_points_device(maps.data_ptr(), w, w * h, 8, pc8.data_ptr(), None, 0)
    ctx.sync()
    cnt8 = pc8.cpu().numpy().view(np.uint32).astype(np.int64)
    pcap = int(cnt8.max())
    pts8 = torch.zeros((8, pcap, 2), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.edge_points_device(maps.data_ptr(), w, w * h, 8, pc8.data_ptr(), pts8.data_ptr(), pcap)
    ctx.sync()
    pts = pts8.repeat((n + 7) // 8, 1, 1)[:n].contiguous()
    pcounts = pc8.repeat((n + 7) // 8)[:n].contiguous()
    cap = 0 if a.counts_only else a.max_lines
    lcounts = torch.zeros((n,), dtype=torch.int32, device="cuda")
    lines = torch.zeros((n, max(cap, 1), 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.set_stream(s.cuda_stream)
    if a.rows:
        ctx.set_option(api.OPT_TEST_HOUGH_ROWS, a.rows)

    def step():
        ctx.hough_lines_device(pts.data_ptr(), pcounts.data_ptr(), pcap, n, rho, theta, a.threshold, 0.0, math.pi, lcounts.data_ptr(),
                               lines.data_ptr() if cap else None, cap)

    for _ in range(a.warmup):
        step()
    ctx.sync()
    s.synchronize()
    times = []
    for _ in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        step()
        e1.record(s)
        ctx.sync()
        s.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    med = times[len(times) // 2]
    numangle, numrho = api.hough_tables(w, h, rho, theta)[:2]
    points = int(np.tile(cnt8, (n + 7) // 8)[:n].sum())
    votes = points * numangle
    res = {"what": "counts" if a.counts_only else "lines", "content": a.content, "frames": n, "threshold": a.threshold, "line_capacity": cap,
           "points_per_frame": round(points / n, 1), "numangle": numangle, "numrho": numrho, "rows_requested": a.rows or None,
           "peaks_per_frame": round(float(lcounts.cpu().numpy().view(np.uint32).mean()), 1),
           "ms_median": round(med, 4), "ms_min": round(times[0], 4), "ms_max": round(times[-1], 4), "ms_per_frame": round(med / n, 4),
           "Gvotes_per_s": round(votes / (med * 1e-3) / 1e9, 2)}
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.record:
        out = os.path.join(ROOT, "profiles", "hough")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "hough_bench.jsonl"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
