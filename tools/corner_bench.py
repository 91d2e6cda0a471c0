#!/usr/bin/env python3
"""Timing of hc_corner_response_device and hc_good_features_device beside hc_derivatives_device and hc_edge_points_device on the
same frames, in the same session.

Usage: tools/corner_bench.py [--steps 20] [--frames 64] [--out FILE]
1080p, `frames` frames per call, the bench's natural and noise contents.  Every timing is between two events on the context's
stream, `steps` timed calls after two warm-up ones, the median with min and max.  The measuring runs in one child process under
`timeout`; a non-zero status ends the script.  JSON lines:
  response   per content: deriv_ms (hc_derivatives_device, ksize 3: k_deriv16, 5 bytes a pixel), response_ms[B][method] and their
             ratio to deriv_ms.  k_corner_response moves 8 bytes a pixel, so 1.6 is the traffic floor of that ratio (`floor`), and
             `over_floor` = ratio / 1.6.  (deriv.hip is older than the corner entries and untouched by them, so k_deriv16 in this
             session is the parent commit's kernel.)
  features   per plane (the min-eigen response of the natural frames, of the noise frames, and a constant positive plane -- every
             interior pixel a candidate, the worst case of the select) and candidate_capacity 1024 / 4096: call_ms at
             quality_level 0.01, min_distance 10, 1000 corners; candidates = local maxima above the threshold (host count of
             frame 0); edge_points_ms: one hc_edge_points_device call on the cv::Canny (60, 150) maps of the same frames, the
             yardstick for a count / scan / emit pipeline over a plane; `noise_over_natural` / `constant_over_natural`: the call against the natural plane's at the same capacity.

tools/corner_bench.py --trace [--frames 64] [--out FILE]: the kernels one by one, in a run of its own under
`rocprofv3 --kernel-trace --stats` (no counters in the same run): ten calls per case after two warm-up calls.  One `trace` line for
k_deriv16 and each k_corner_response<B, method> per content, and one per features case with the median microseconds of each kernel
of a call and the three sums `plane_us` (k_feat_max + the five k_feat_plane walks), `rank_us` and `sift_us`."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1920, 1080
BLOCKS = (3, 5, 7)
CAPS = (1024, 4096)
TRACE_CALLS = 10
FLOOR = 1.6


def _setup(n):
    """context, the int16 planes of both contents, the three response planes and the Canny maps (all on the device)"""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from cudacam_amd import api, synth
    fs = W * H
    ctx = api.Context(W, H, 1, n, api.MODE_O)
    distinct = min(8, n)
    reps = (n + distinct - 1) // distinct
    data = {}
    for content in ("natural", "noise"):
        frames = synth.frames(content, W, H, distinct, seed=synth.SEED0 + 77)
        src = torch.from_numpy(np.ascontiguousarray(frames)).cuda().repeat((reps, 1, 1))[:n].contiguous()
        gx, gy = torch.empty((n, H, W), dtype=torch.int16, device="cuda"), torch.empty((n, H, W), dtype=torch.int16, device="cuda")
        resp = torch.empty((n, H, W), dtype=torch.float32, device="cuda")
        maps = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.derivatives_device(src.data_ptr(), W, fs, gx.data_ptr(), gy.data_ptr(), 2 * W, 2 * fs, n, 3)
        ctx.corner_response_device(gx.data_ptr(), gy.data_ptr(), 2 * W, 2 * fs, resp.data_ptr(), 4 * W, 4 * fs, n, 3, api.CORNER_MIN_EIGEN, 0.04)
        ctx.canny_device(src.data_ptr(), W, fs, maps.data_ptr(), W, fs, n, 60, 150, 3, False)
        ctx.sync()
        data[content] = dict(src=src, gx=gx, gy=gy, resp=resp, maps=maps)
    data["constant"] = dict(resp=torch.full((n, H, W), 3.25, dtype=torch.float32, device="cuda"), maps=data["natural"]["maps"])
    torch.cuda.synchronize()
    return ctx, api, data


def _host_candidates(plane, q):
    """local maxima above the threshold of one float32 frame (numpy; the rule of include/hipcanny.h)"""
    import numpy as np
    bits = np.ascontiguousarray(plane).view(np.uint32)
    k = np.where((bits.view(np.int32) > 0) & (bits <= 0x7F800000), bits, 0).astype(np.uint32)
    m = np.uint32(k.max()).reshape(1).view(np.float32)[0]
    t = np.float32(m * np.float32(q))
    tk = int(t.reshape(1).view(np.uint32)[0]) if t > 0 else 0
    c = k[1:-1, 1:-1]
    nb = np.zeros_like(c)
    for dy in range(3):
        for dx in range(3):
            if (dy, dx) != (1, 1):
                nb = np.maximum(nb, k[dy:dy + H - 2, dx:dx + W - 2])
    return int(((c > tk) & (c >= nb)).sum())


def child(n, steps):
    import torch
    ctx, api, data = _setup(n)
    fs = W * H
    ctx.set_stream(0)   # the null stream: torch's events bracket the call
    torch.cuda.synchronize()

    def timed(run):
        for _ in range(2):
            run()
        torch.cuda.synchronize()
        ms = []
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms.sort()
        return [round(ms[len(ms) // 2], 4), round(ms[0], 4), round(ms[-1], 4)]

    for content in ("natural", "noise"):
        d = data[content]
        out = torch.empty((n, H, W), dtype=torch.float32, device="cuda")
        deriv = timed(lambda: ctx.derivatives_device(d["src"].data_ptr(), W, fs, d["gx"].data_ptr(), d["gy"].data_ptr(), 2 * W, 2 * fs, n, 3))
        res = {"response": content, "frames": n, "steps": steps, "deriv_ms": deriv, "floor": FLOOR, "response_ms": {}, "ratio": {}, "over_floor": {}}
        for B in BLOCKS:
            for mname, method in api.CORNER_METHODS.items():
                t = timed(lambda: ctx.corner_response_device(d["gx"].data_ptr(), d["gy"].data_ptr(), 2 * W, 2 * fs, out.data_ptr(), 4 * W, 4 * fs, n, B, method, 0.04))
                key = f"{B}_{mname}"
                res["response_ms"][key] = t
                res["ratio"][key] = round(t[0] / deriv[0], 3)
                res["over_floor"][key] = round(t[0] / deriv[0] / FLOOR, 3)
        print(json.dumps(res), flush=True)
        del out
    counts = torch.empty((n,), dtype=torch.int32, device="cuda")
    corners = torch.empty((n, 1000, 2), dtype=torch.float32, device="cuda")
    pcounts = torch.empty((n,), dtype=torch.int32, device="cuda")
    natural = {}
    for plane in ("natural", "noise", "constant"):
        d = data[plane]
        ctx.edge_points_device(d["maps"].data_ptr(), W, fs, n, pcounts.data_ptr(), None, 0)
        torch.cuda.synchronize()
        pcap = max(int(pcounts.cpu().numpy().max()), 1)
        pts = torch.empty((n, pcap, 2), dtype=torch.int32, device="cuda")
        edge = timed(lambda: ctx.edge_points_device(d["maps"].data_ptr(), W, fs, n, pcounts.data_ptr(), pts.data_ptr(), pcap))
        cands = _host_candidates(d["resp"][0].cpu().numpy(), 0.01)
        for cap in CAPS:
            t = timed(lambda: ctx.good_features_device(d["resp"].data_ptr(), 4 * W, 4 * fs, n, 0.01, 10.0, cap, counts.data_ptr(), corners.data_ptr(), None, 1000))
            kept = counts.cpu().numpy()
            res = {"features": plane, "candidate_capacity": cap, "frames": n, "steps": steps, "candidates_frame0": cands, "kept_min_max": [int(kept.min()), int(kept.max())],
                   "call_ms": t, "edge_points_ms": edge, "edge_points": pcap, "call_over_edge_points": round(t[0] / edge[0], 3)}
            if plane == "natural":
                natural[cap] = t[0]
            else:
                res[plane + "_over_natural"] = round(t[0] / natural[cap], 3)
            print(json.dumps(res), flush=True)
        del pts
    ctx.use_own_stream()
    ctx.close()


def trace_child(n):
    import torch
    ctx, api, data = _setup(n)
    fs = W * H
    out = torch.empty((n, H, W), dtype=torch.float32, device="cuda")
    counts = torch.empty((n,), dtype=torch.int32, device="cuda")
    corners = torch.empty((n, 1000, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    order = []
    for content in ("natural", "noise"):
        d = data[content]
        for _ in range(2 + TRACE_CALLS):
            ctx.derivatives_device(d["src"].data_ptr(), W, fs, d["gx"].data_ptr(), d["gy"].data_ptr(), 2 * W, 2 * fs, n, 3)
            ctx.sync()
        for B in (3, 7):
            for mname, method in api.CORNER_METHODS.items():
                for _ in range(2 + TRACE_CALLS):
                    ctx.corner_response_device(d["gx"].data_ptr(), d["gy"].data_ptr(), 2 * W, 2 * fs, out.data_ptr(), 4 * W, 4 * fs, n, B, method, 0.04)
                    ctx.sync()
    for plane in ("natural", "noise", "constant"):
        for cap in CAPS:
            order.append([plane, cap])
            for _ in range(2 + TRACE_CALLS):
                ctx.good_features_device(data[plane]["resp"].data_ptr(), 4 * W, 4 * fs, n, 0.01, 10.0, cap, counts.data_ptr(), corners.data_ptr(), None, 1000)
                ctx.sync()
    ctx.close()
    print(json.dumps({"trace_order": order, "frames": n}), flush=True)


def trace_lines(csv_path, info):
    """The `trace` lines from a rocprofv3 kernel-trace CSV (rows with Kernel_Name, Start_Timestamp, End_Timestamp in ns)."""
    import csv
    import re
    import statistics
    rows = sorted(csv.DictReader(open(csv_path)), key=lambda r: int(r["Start_Timestamp"]))
    per = 2 + TRACE_CALLS
    deriv, resp, feat, cur = [], {}, [], None
    for r in rows:
        name, us = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        m = re.search(r"k_corner_response<\s*(\d)\s*,\s*(\d)\s*>", name) or re.search(r"k_corner_responseILi(\d)ELi(\d)E", name)
        if "k_deriv16" in name:
            deriv.append(us)
        elif m:
            resp.setdefault((int(m.group(1)), int(m.group(2))), []).append(us)
        elif "k_feat_max" in name:
            cur = {"k_feat_max": us}
            feat.append(cur)   # (a call is k_feat_max and the twelve launches behind it; the set-up makes no such call)
        elif "k_feat_" in name and cur is not None:
            short = re.search(r"k_feat_[a-z]+", name).group(0)
            cur[short] = cur.get(short, 0.0) + us
    med = lambda v: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "dispatches": len(v)}
    out = []
    deriv = deriv[-2 * per:]   # (the launches before them are the set-up)
    for ci, content in enumerate(("natural", "noise")):
        dv = deriv[ci * per + 2:(ci + 1) * per]
        if dv:
            out.append(json.dumps({"trace": f"{content}_k_deriv16_ksize3", "frames": info["frames"], "us": med(dv)}))
        for (B, method), v in sorted(resp.items()):
            mine = v[-2 * per:][ci * per + 2:(ci + 1) * per]
            if mine and dv:
                ratio = statistics.median(mine) / statistics.median(dv)
                out.append(json.dumps({"trace": f"{content}_k_corner_response_B{B}_{'harris' if method else 'min_eigen'}", "frames": info["frames"], "us": med(mine),
                                       "ratio_to_deriv": round(ratio, 3), "over_floor": round(ratio / FLOOR, 3)}))
    for k, (plane, cap) in enumerate(info["trace_order"]):
        mine = feat[k * per + 2:(k + 1) * per]
        if not mine:
            continue
        kernels = sorted({n for c in mine for n in c})
        res = {"trace": f"features_{plane}_{cap}", "frames": info["frames"], "calls": len(mine), "kernel_us": {n: round(statistics.median(c.get(n, 0.0) for c in mine), 2) for n in kernels}}
        res["plane_us"] = round(res["kernel_us"].get("k_feat_max", 0) + res["kernel_us"].get("k_feat_plane", 0), 2)
        res["rank_us"], res["sift_us"] = res["kernel_us"].get("k_feat_rank", 0), res["kernel_us"].get("k_feat_sift", 0)
        res["kernels_per_call_us"] = round(statistics.median(sum(c.values()) for c in mine), 2)
        out.append(json.dumps(res))
    return out


def trace(a):
    import glob
    import shutil
    import tempfile
    out_dir = os.path.dirname(os.path.abspath(a.out)) if a.out else tempfile.gettempdir()
    os.makedirs(out_dir, exist_ok=True)
    d = os.path.join(out_dir, "corner_trace_tmp")
    shutil.rmtree(d, ignore_errors=True)
    cmd = ["timeout", "-k", "10", "400", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--trace-child",
           "--frames", str(a.frames)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=tempfile.gettempdir())
    info = [l for l in r.stdout.splitlines() if l.startswith('{"trace_order"')]
    if r.returncode != 0 or not info:
        print(f"exit {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}", file=sys.stderr, flush=True)
        sys.exit(1)   # nothing more is started on the GPU
    files = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
    if not files:
        sys.exit("no kernel trace was written")
    lines = trace_lines(max(files, key=os.path.getsize), json.loads(info[-1]))
    shutil.rmtree(d, ignore_errors=True)
    print("\n".join(lines), flush=True)
    if a.out and lines:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corners", "corner_bench.jsonl"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--trace", action="store_true", help="the kernels one by one from a rocprofv3 kernel trace, in a run of its own")
    ap.add_argument("--trace-child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.frames, a.steps)
        return
    if a.trace_child:
        trace_child(a.frames)
        return
    if a.trace:
        if a.out == ap.get_default("out"):
            a.out = os.path.join(ROOT, "profiles", "corners", "corner_trace.jsonl")
        trace(a)
        return
    cmd = ["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps), "--frames", str(a.frames)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    print("\n".join(lines), flush=True)
    if a.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if r.returncode != 0:
        print(f"exit {r.returncode}\n{r.stderr[-3000:]}", file=sys.stderr, flush=True)
        sys.exit(1)   # nothing more is started on the GPU


if __name__ == "__main__":
    main()
