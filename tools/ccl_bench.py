"""Times hc_connected_components_device over the C ABI (profiles/ccl/README.md):

    python tools/ccl_bench.py [--content natural,noise,full] [--connectivity 4,8] [--frames N] [--labels-only] [--check] [--cpu]

1920 x 1080 maps.  natural / noise: cv::Canny's maps (Mode O, canny_device, thresholds 50 / 150, aperture 3) of synth's natural
and noise frames, 4 distinct frames repeated on the device to `frames`; full: every pixel set.  capacity = the largest count, so
every row is written (--labels-only: capacity 0, the three statistics kernels are not launched).  All launches of a call together
are timed with events on the stream the context runs on, and beside them hc_edge_points_device with capacity 0 over the same maps
(k_edge_count and k_edge_scan: the cost of reading the maps once).  --check compares the first 4 frames with scipy.ndimage.label
(labels, counts) and tests/ccl_ref.py's statistics; --cpu times scipy.ndimage.label on one map on this machine's CPU.  Prints one
JSON line per (content, connectivity), and appends them to profiles/ccl/ccl_bench.jsonl with --record.  Per-kernel times come
from running this tool under a kernel trace with one content and one connectivity."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cudacam_amd import api, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--content", default="natural,noise,full")
    ap.add_argument("--connectivity", default="4,8")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--labels-only", action="store_true", help="capacity 0: labels and counts only")
    ap.add_argument("--check", action="store_true", help="compare the distinct frames with scipy.ndimage.label and tests/ccl_ref.py")
    ap.add_argument("--cpu", action="store_true", help="time scipy.ndimage.label on one map on the CPU")
    ap.add_argument("--record", action="store_true", help="append the results to profiles/ccl/ccl_bench.jsonl")
    a = ap.parse_args()
    import torch
    w, h, n, k = 1920, 1080, a.frames, 4
    s = torch.cuda.Stream()
    ctx = api.Context(w, h, 1, max(n, k), api.MODE_O)
    reps = (n + k - 1) // k
    lines = []
    for content in a.content.split(","):
        if content == "full":
            mapsk = torch.full((k, h, w), 255, dtype=torch.uint8, device="cuda")
        else:
            src = torch.from_numpy(synth.frames(content, w, h, k, seed=synth.SEED0 + 9000)).cuda()
            mapsk = torch.empty((k, h, w), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ctx.canny_device(src.data_ptr(), w, w * h, mapsk.data_ptr(), w, w * h, k, 50, 150)
            ctx.sync()
        maps = mapsk.repeat(reps, 1, 1)[:n].contiguous()
        host = mapsk.cpu().numpy()
        labels = torch.empty((n, h, w), dtype=torch.int32, device="cuda")
        counts = torch.zeros((n,), dtype=torch.int32, device="cuda")
        pcounts = torch.zeros((n,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for conn in (int(v) for v in a.connectivity.split(",")):
            ctx.use_own_stream()
            ctx.connected_components_device(maps.data_ptr(), w, w * h, n, conn, labels.data_ptr(), 4 * w, 4 * w * h, counts.data_ptr())
            ctx.sync()
            cnt = counts.cpu().numpy().view(np.uint32).astype(np.int64)
            cap = 0 if a.labels_only else int(cnt.max())
            stats = torch.zeros((n, max(cap, 1), 5), dtype=torch.int32, device="cuda")
            cents = torch.zeros((n, max(cap, 1), 2), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            ctx.set_stream(s.cuda_stream)

            def ccl():
                ctx.connected_components_device(maps.data_ptr(), w, w * h, n, conn, labels.data_ptr(), 4 * w, 4 * w * h, counts.data_ptr(),
                                                stats.data_ptr() if cap else None, cents.data_ptr() if cap else None, cap)

            def read_once():
                ctx.edge_points_device(maps.data_ptr(), w, w * h, n, pcounts.data_ptr(), None, 0)

            med = {}
            for name, step in (("ccl", ccl), ("edge_count", read_once)):
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
                med[name] = (times[len(times) // 2], times[0], times[-1])
            res = {"what": "labels" if a.labels_only else "labels+stats", "content": content, "connectivity": conn, "frames": n, "capacity": cap,
                   "pixels_set_per_frame": round(float(pcounts.cpu().numpy().view(np.uint32).mean()), 1), "components_per_frame": round(float(cnt.mean()) - 1, 1),
                   "ms_median": round(med["ccl"][0], 4), "ms_min": round(med["ccl"][1], 4), "ms_max": round(med["ccl"][2], 4), "ms_per_frame": round(med["ccl"][0] / n, 4),
                   "edge_count_ms_median": round(med["edge_count"][0], 4), "edge_count_ms_per_frame": round(med["edge_count"][0] / n, 4)}
            if a.check or a.cpu:
                import scipy.ndimage as ndi
                structure = np.ones((3, 3), int) if conn == 8 else None
                t0 = time.perf_counter()
                want0, k0 = ndi.label(host[0] != 0, structure)
                res["scipy_label_ms_per_frame"] = round(1e3 * (time.perf_counter() - t0), 2)
            if a.check:
                import ccl_ref as R
                got, gs, gc = labels[:k].cpu().numpy(), stats[:k].cpu().numpy(), cents[:k].cpu().numpy()
                ok = True
                for f in range(k):
                    want, kf = ndi.label(host[f] != 0, structure)
                    ok = ok and int(cnt[f]) == kf + 1 and np.array_equal(got[f], want)
                    if cap:
                        st, cen = R.stats_fast(want.astype(np.int32), kf + 1)
                        ok = ok and np.array_equal(gs[f, :kf + 1], st) and np.array_equal(gc[f, :kf + 1].view(np.int64), cen.view(np.int64))
                res["equals_scipy"] = bool(ok)
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
    ctx.close()
    if a.record:
        out = os.path.join(ROOT, "profiles", "ccl")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "ccl_bench.jsonl"), "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
