"""Times hc_hough_circles_device over the C ABI (profiles/hough_circles/README.md):

    python tools/hough_circles_bench.py --content drawn|noise [--frames N] [--threshold T] [--dp DP] [--min-dist D] [--counts-only]

1920 x 1080 frames.  drawn: discs of radius 12 .. 95 on a flat background with a little noise; noise: bench.py's noise generator.
The point lists are hc_edge_points_device's of cv::Canny's maps (Mode O, canny_device, thresholds 50 / 150, aperture 3), the
gradient planes hc_derivatives_device's (ksize 3) of the same frames: 4 distinct frames, repeated on the device to `frames`;
point_capacity = the largest count, so nothing is cut.  min_radius .. max_radius = 10 .. 100.  All launches of a call together
are timed with events on the stream the context runs on (--counts-only: circle_capacity 0, one k_circle_radii launch); one
measurement per process.  Prints one JSON line, and appends it to profiles/hough_circles/hough_circles_bench.jsonl with --record.
Per-kernel times come from running this tool under a kernel trace; --steps then sets the number of calls traced."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cudacam_amd import api, synth  # noqa: E402


def drawn(w, h, seed):
    rng = np.random.default_rng(seed)
    f = np.full((h, w), 40, np.int16)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(24):
        cx, cy, r = int(rng.integers(0, w)), int(rng.integers(0, h)), int(rng.integers(12, 96))
        f[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = int(rng.integers(90, 250))
    return np.clip(f + rng.integers(-3, 4, (h, w)), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--content", default="drawn", choices=["drawn", "noise"])
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--threshold", type=int, default=40)
    ap.add_argument("--dp", type=float, default=1.0)
    ap.add_argument("--min-dist", type=float, default=20.0)
    ap.add_argument("--max-centres", type=int, default=4096)
    ap.add_argument("--max-circles", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--counts-only", action="store_true", help="circle_capacity 0: no emit pass")
    ap.add_argument("--record", action="store_true", help="append the result to profiles/hough_circles/hough_circles_bench.jsonl")
    a = ap.parse_args()
    import torch
    w, h, n, k = 1920, 1080, a.frames, 4
    rmin, rmax = 10, 100
    src = np.stack([drawn(w, h, 500 + i) for i in range(k)]) if a.content == "drawn" else synth.frames("noise", w, h, k, seed=synth.SEED0 + 9000)
    s = torch.cuda.Stream()
    ctx = api.Context(w, h, 1, max(n, k), api.MODE_O)
    d_src = torch.from_numpy(src).cuda()
    maps = torch.empty((k, h, w), dtype=torch.uint8, device="cuda")
    gx, gy = torch.empty((k, h, w), dtype=torch.int16, device="cuda"), torch.empty((k, h, w), dtype=torch.int16, device="cuda")
    pck = torch.zeros((k,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.derivatives_device(d_src.data_ptr(), w, w * h, gx.data_ptr(), gy.data_ptr(), 2 * w, 2 * w * h, k, 3)
    ctx.canny_device(d_src.data_ptr(), w, w * h, maps.data_ptr(), w, w * h, k, 50, 150)
    ctx.edge_points_device(maps.data_ptr(), w, w * h, k, pck.data_ptr(), None, 0)
    ctx.sync()
    cntk = pck.cpu().numpy().view(np.uint32).astype(np.int64)
    pcap = max(int(cntk.max()), 1)
    ptsk = torch.zeros((k, pcap, 2), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.edge_points_device(maps.data_ptr(), w, w * h, k, pck.data_ptr(), ptsk.data_ptr(), pcap)
    ctx.sync()
    reps = (n + k - 1) // k
    pts, pcounts = ptsk.repeat(reps, 1, 1)[:n].contiguous(), pck.repeat(reps)[:n].contiguous()
    dx, dy = gx.repeat(reps, 1, 1)[:n].contiguous(), gy.repeat(reps, 1, 1)[:n].contiguous()
    cap = 0 if a.counts_only else a.max_circles
    ccounts = torch.zeros((n,), dtype=torch.int32, device="cuda")
    circles = torch.zeros((n, max(cap, 1), 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.set_stream(s.cuda_stream)

    def step():
        ctx.hough_circles_device(pts.data_ptr(), pcounts.data_ptr(), pcap, dx.data_ptr(), dy.data_ptr(), 2 * w, 2 * w * h, n, a.dp, a.min_dist, a.threshold,
                                 rmin, rmax, a.max_centres, ccounts.data_ptr(), circles.data_ptr() if cap else None, cap)

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
    aw, ah, min_d2 = api.hough_circle_geometry(w, h, a.dp, a.min_dist, rmin, rmax)
    res = {"what": "counts" if a.counts_only else "circles", "content": a.content, "frames": n, "threshold": a.threshold, "dp": a.dp, "min_dist": a.min_dist,
           "centre_capacity": a.max_centres, "circle_capacity": cap, "radii": [rmin, rmax], "points_per_frame": round(float(np.tile(cntk, reps)[:n].mean()), 1),
           "acc": [aw, ah], "min_d2": min_d2, "circles_per_frame": round(float(ccounts.cpu().numpy().view(np.uint32).mean()), 1),
           "ms_median": round(med, 4), "ms_min": round(times[0], 4), "ms_max": round(times[-1], 4), "ms_per_frame": round(med / n, 4)}
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.record:
        out = os.path.join(ROOT, "profiles", "hough_circles")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "hough_circles_bench.jsonl"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
