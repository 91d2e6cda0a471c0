"""Times hc_edge_points_device over the C ABI (profiles/edge_points/README.md):

    python tools/edge_points_bench.py --content natural|noise [--counts-only]

The maps are cv::Canny's (Mode O, canny_device, thresholds 50 / 150, aperture 3) of bench.py's generators: 8 distinct frames of
synth.frames at bench.py's seeds, their maps repeated on the device to 1024 maps of 1920 x 1080.  capacity = the largest count,
so nothing is cut.  The three launches together are timed with events on the stream the context runs on; one measurement per
process; prints one JSON line with the times, the edge density and the traffic floor (2 x map bytes read + 8 B per point
written -- one read and no list with --counts-only -- at the copy rate the project's roofline uses, 6.29 TB/s)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cudacam_amd import api, synth  # noqa: E402

COPY_TB_PER_S = 6.29   # measured float4 copy rate of the MI355X (profiles/auto_thr/README.md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--content", default="natural", choices=["natural", "noise"])
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--counts-only", action="store_true", help="capacity 0: k_edge_count and k_edge_scan only (cv::countNonZero)")
    a = ap.parse_args()
    import torch
    w, h, n = a.width, a.height, a.frames
    src = synth.frames(a.content, w, h, 8, seed=synth.SEED0 + (9000 if a.content == "noise" else 0))
    s = torch.cuda.Stream()
    ctx = api.Context(w, h, 1, n, api.MODE_O)
    base = torch.from_numpy(ctx.canny(src, 50, 150)).cuda()
    maps = base.repeat((n + 7) // 8, 1, 1)[:n].contiguous()
    counts = torch.zeros((n,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.set_stream(s.cuda_stream)
    ctx.edge_points_device(maps.data_ptr(), w, w * h, n, counts.data_ptr(), None, 0)
    ctx.sync()
    s.synchronize()
    cnt = counts.cpu().numpy().view(np.uint32).astype(np.int64)
    cap = 0 if a.counts_only else int(cnt.max())
    pts = torch.zeros((n, max(cap, 1), 2), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def step():
        ctx.edge_points_device(maps.data_ptr(), w, w * h, n, counts.data_ptr(), pts.data_ptr() if cap else None, cap)

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
    host = base.cpu().numpy()
    exact = cnt[:8].tolist() == [int((m != 0).sum()) for m in host]
    if cap:
        got = pts[:8].cpu().numpy()
        exact = exact and all(np.array_equal(got[f, :cnt[f]], np.argwhere(host[f] != 0)[:, ::-1].astype(np.int32)) for f in range(8))
    map_bytes, points = n * w * h, int(cnt.sum())
    traffic = (1 if a.counts_only else 2) * map_bytes + (0 if a.counts_only else 8 * points)
    floor_ms = traffic / (COPY_TB_PER_S * 1e12) * 1e3
    res = {"what": "counts" if a.counts_only else "points", "content": a.content, "frames": n, "width": w, "height": h,
           "density": round(points / map_bytes, 5), "points": points, "capacity": cap,
           "ms_median": round(med, 4), "ms_min": round(times[0], 4), "ms_max": round(times[-1], 4),
           "traffic_GB": round(traffic / 1e9, 3), "floor_ms": round(floor_ms, 4), "floor_over_time": round(floor_ms / med, 3),
           "traffic_TB_per_s": round(traffic / (med * 1e-3) / 1e12, 3), "exact": bool(exact)}
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
