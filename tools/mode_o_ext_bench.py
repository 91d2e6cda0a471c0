#!/usr/bin/env python3
"""Front-kernel timing of Mode O's k_front_o_ext (aperture 5, given gradients) beside k_front_o and k_front8o.

Usage: tools/mode_o_ext_bench.py [--steps 20] [--frames 512] [--out FILE]
Every configuration runs in a fresh process under `timeout`: 1080p, 512 frames per launch (3-channel: 256), `steps` timed
launches after two warm-up ones.  Reports the front kernel's median ms (hc_profile_get_front_each), frames/s of the front
kernel alone and of pipelined runs (HC_OPT_PIPELINE, end-to-end), and the fraction of 6.29 TB/s that the kernel's own
bytes make at the median: 1 B/px (3 B/px BGR) of input + 0.25 B/px of bit planes for the u8 forms, 4 C B/px + 0.25 for
the gradient form."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM = 6.29e12
W, H = 1920, 1080
CONFIGS = [  # name, channels, form
    ("gradients_mono", 1, "grad"), ("aperture5_mono", 1, "ap5"), ("k_front_o_mono", 1, "fo"), ("k_front8o_mono", 1, "f8o"),
    ("gradients_bgr", 3, "grad"), ("aperture5_bgr", 3, "ap5"), ("k_front_o_bgr", 3, "fo"),
]


def child(name, ch, form, n, steps):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from cudacam_amd import api, synth
    import canny_o_ext_ref as X
    distinct = 8
    base = [synth.natural(W, H, 100 + k) for k in range(distinct)]
    if ch == 3:
        base = [np.stack([b, b[::-1].copy(), b[:, ::-1].copy()], -1) for b in base]
    reps = (n + distinct - 1) // distinct
    low, high = (300, 900) if form == "ap5" else (50, 150)
    ctx = api.Context(W, H, ch, n, api.MODE_O)
    ctx.set_thresholds(low, high)
    if form == "ap5":
        ctx.set_option(api.OPT_APERTURE, 5)
    if form == "fo":
        ctx.set_option(api.OPT_FRONT_SPLIT, 0)
    out = [torch.empty((n, H, W), dtype=torch.uint8, device="cuda") for _ in range(4)]
    if form == "grad":
        g = [X.sobel_o(b, 3) for b in base]
        dx = torch.from_numpy(np.stack([a for a, _ in g]).astype(np.int16)).cuda().repeat((reps,) + (1,) * (g[0][0].ndim))[:n].contiguous()
        dy = torch.from_numpy(np.stack([b for _, b in g]).astype(np.int16)).cuda().repeat((reps,) + (1,) * (g[0][0].ndim))[:n].contiguous()
        pitch = 2 * ch * W

        def run(o):
            ctx.run_gradients_device(dx.data_ptr(), dy.data_ptr(), pitch, pitch * H, o.data_ptr(), W, W * H, n)
        bytes_px = 4 * ch + 0.25
    else:
        src = torch.from_numpy(np.stack(base)).cuda().repeat((reps,) + (1,) * (base[0].ndim))[:n].contiguous()

        def run(o):
            ctx.run_device(src.data_ptr(), ch * W, ch * W * H, o.data_ptr(), W, W * H, n)
        bytes_px = ch + 0.25
    torch.cuda.synchronize()
    ctx.enable_profiling(1)
    for _ in range(2):
        run(out[0])
    ctx.sync()
    ctx.profile_get(reset=True)
    for s in range(steps):
        run(out[0])
        ctx.sync()
    fe = sorted(ctx.profile_front_each())
    form_id = ctx.last_run_info()[2]
    ctx.enable_profiling(0)
    med = fe[len(fe) // 2]
    # pipelined: back-to-back runs to rotating outputs, wall clock over the steps
    ctx.set_option(api.OPT_PIPELINE, 1)
    depth = max(1, ctx.pipeline_depth(n))
    for k in range(2):
        run(out[k % depth])
    ctx.sync()
    t0 = time.perf_counter()
    for s in range(steps):
        run(out[s % depth])
    ctx.sync()
    dt = (time.perf_counter() - t0) / steps
    ctx.close()
    px = n * W * H
    return {"config": name, "form": form_id, "channels": ch, "frames": n, "steps": steps, "front_ms_median": round(med, 4),
            "front_ms_min": round(fe[0], 4), "front_ms_max": round(fe[-1], 4), "frames_per_s_front": round(n / (med / 1e3)),
            "frames_per_s_pipelined": round(n / dt), "bytes_per_px": bytes_px, "frac_hbm": round(px * bytes_px / (med / 1e3) / HBM, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        name, ch, form = next(c for c in CONFIGS if c[0] == a.child)
        n = a.frames if ch == 1 else a.frames // 2
        print(json.dumps(child(name, ch, form, n, a.steps)), flush=True)
        return
    lines = []
    for name, ch, form in CONFIGS:
        if a.only and name not in a.only.split(","):
            continue
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", name, "--steps", str(a.steps),
               "--frames", str(a.frames)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        res = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0 or not res:
            print(f"{name}: exit {r.returncode}\n{r.stderr[-2000:]}", file=sys.stderr, flush=True)
            if r.returncode in (124, 137, 134, 139, -6, -11):
                break   # a fault or a hang: start nothing more on the GPU
            continue
        print(res[-1], flush=True)
        lines.append(res[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
