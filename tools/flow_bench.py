#!/usr/bin/env python3
"""Timing of hc_pyr_down_device and hc_lk_flow_device beside hc_gaussian_blur_device and hc_good_features_device on the same frames,
in the same session.

Usage: tools/flow_bench.py [--frames 64] [--features 1024] [--out FILE]
1080p, `frames` frames per call, the bench's natural content and the same frames shifted by (3, 2) pixels; the points are the
`features` strongest corners a frame from Context's feature chain (min-eigen, block 3, quality 0.01, distance 10).  The measuring
runs in one child process under `rocprofv3 --kernel-trace --stats` (no counters in the same run) and `timeout`: CALLS calls per case
after two warm-up calls; a non-zero status ends the script.  One JSON line per kernel name with the median, the smallest and the
largest microseconds of a launch: k_gauss8 (5 x 5, the yardstick of k_pyr_down8, which reads the same bytes and writes a quarter),
k_pyr_down8 at level 0 -> 1, k_lk_flow<rounds> per window (level 0, 30 iterations, epsilon 0.01) and the kernels of the
hc_good_features_device call that produced the points, summed per call as `features_call_us`."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1920, 1080
WINS = (7, 15, 21, 31)
CALLS = 10


def trace_child(n, cap):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from cudacam_amd import api, synth
    fs = W * H
    ctx = api.Context(W, H, 1, n, api.MODE_O)
    distinct = min(8, n)
    reps = (n + distinct - 1) // distinct
    frames = np.ascontiguousarray(synth.frames("natural", W, H, distinct, seed=synth.SEED0 + 77))
    a = torch.from_numpy(frames).cuda().repeat((reps, 1, 1))[:n].contiguous()
    b = torch.roll(a, (2, 3), (1, 2)).contiguous()
    gx, gy = torch.empty((n, H, W), dtype=torch.int16, device="cuda"), torch.empty((n, H, W), dtype=torch.int16, device="cuda")
    resp = torch.empty((n, H, W), dtype=torch.float32, device="cuda")
    blur = torch.empty_like(a)
    half = torch.empty((n, H // 2, W // 2), dtype=torch.uint8, device="cuda")
    counts = torch.zeros((n,), dtype=torch.int32, device="cuda")
    pts = torch.zeros((n, cap, 2), dtype=torch.float32, device="cuda")
    nxt = torch.zeros_like(pts)
    status = torch.zeros((n, cap), dtype=torch.uint8, device="cuda")
    err = torch.zeros((n, cap), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.derivatives_device(a.data_ptr(), W, fs, gx.data_ptr(), gy.data_ptr(), 2 * W, 2 * fs, n, 3)
    ctx.corner_response_device(gx.data_ptr(), gy.data_ptr(), 2 * W, 2 * fs, resp.data_ptr(), 4 * W, 4 * fs, n, 3, api.CORNER_MIN_EIGEN, 0.04)
    ctx.sync()
    taps = api.gaussian_taps_q8(5, 0.0)
    for _ in range(2 + CALLS):
        ctx.good_features_device(resp.data_ptr(), 4 * W, 4 * fs, n, 0.01, 10.0, 4096, counts.data_ptr(), pts.data_ptr(), None, cap)
        ctx.gaussian_blur_device(a.data_ptr(), W, fs, blur.data_ptr(), W, fs, n, 5, taps)
        ctx.pyr_down_device(a.data_ptr(), W, fs, W, H, half.data_ptr(), W // 2, (W // 2) * (H // 2), n)
        for win in WINS:
            ctx.lk_flow_device(a.data_ptr(), b.data_ptr(), W, fs, W, H, 0, n, counts.data_ptr(), pts.data_ptr(), nxt.data_ptr(), cap, win, 30, 0.01, 1e-4, 0, status.data_ptr(),
                               err.data_ptr())
        ctx.sync()
    c = counts.cpu().numpy()
    print(json.dumps({"trace_info": 1, "frames": n, "capacity": cap, "points_min": int(c.min()), "points_max": int(c.max()), "tracked": int(status.sum().item())}), flush=True)


def trace(a):
    import csv
    import glob
    import shutil
    import tempfile
    out_dir = os.path.dirname(os.path.abspath(a.out))
    os.makedirs(out_dir, exist_ok=True)
    d = os.path.join(out_dir, "flow_trace_tmp")
    shutil.rmtree(d, ignore_errors=True)
    cmd = ["timeout", "-k", "10", "400", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--trace-child",
           "--frames", str(a.frames), "--features", str(a.features)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=tempfile.gettempdir())
    info = [l for l in r.stdout.splitlines() if l.startswith('{"trace_info"')]
    if r.returncode != 0 or not info:
        print(f"exit {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}", file=sys.stderr, flush=True)
        sys.exit(1)   # nothing more is started on the GPU
    files = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
    if not files:
        sys.exit("no kernel trace was written")
    by = {}
    for row in csv.DictReader(open(max(files, key=os.path.getsize))):
        name = row["Kernel_Name"]
        for key in ("k_gauss8", "k_pyr_down8", "k_lk_flow", "k_feat_"):
            if key in name:
                short = name[name.index(key):].split("(")[0]
                by.setdefault(short, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1000.0)
    lines = [info[-1]]
    feat = 0.0
    for name in sorted(by):
        v = sorted(by[name])
        per_call = len(v) // (2 + CALLS)
        v = sorted(by[name][2 * per_call:])   # the warm-up calls come first in a kernel's own order
        lines.append(json.dumps({"kernel": name, "launches_per_call": per_call, "us": [round(v[len(v) // 2], 1), round(v[0], 1), round(v[-1], 1)]}))
        if name.startswith("k_feat_"):
            feat += sum(v) / CALLS
    lines.append(json.dumps({"features_call_us": round(feat, 1)}))
    shutil.rmtree(d, ignore_errors=True)
    print("\n".join(lines), flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--features", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow", "flow_trace.jsonl"))
    ap.add_argument("--trace-child", action="store_true")
    a = ap.parse_args()
    if a.trace_child:
        trace_child(a.frames, a.features)
    else:
        trace(a)


if __name__ == "__main__":
    main()
