#!/usr/bin/env python3
"""Timing of k_gauss8 (hc_gaussian_blur_device) beside its yardstick, k_deriv16 (hc_derivatives_device) in the same session,
and of the chain blur -> cv::Canny beside cv::Canny alone.

Usage: tools/blur_bench.py [--steps 20] [--frames 512] [--only a,b] [--out FILE]
Every configuration runs in a fresh process under `timeout`: 1080p, 512 frames per launch (3-channel: 256), `steps` timed
launches after two warm-up ones, median.
  blur_<ksize>_<mono|bgr>    the kernel alone (sigma 1.4, reflect-101), between two events on the context's stream; its own
                             bytes are C B/px of input + C B/px of output = 2 C B/px
  deriv_<ksize>_<mono|bgr>   k_deriv16 alone, the same way: 5 C B/px.  deriv_7 of the same channel count is what every blur
                             leg must not exceed
  canny3_mono                hc_canny_device at aperture 3, pipelined, wall clock: frames/s
  blur5_canny3_mono          hc_gaussian_blur_device (5, sigma 1.4) + hc_canny_device, pipelined, wall clock: frames/s
Fractions are of 6.29 TB/s at the median."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM = 6.29e12
W, H = 1920, 1080
CONFIGS = ([(f"{form}_{k}_{'mono' if ch == 1 else 'bgr'}", ch, form, k) for ch in (1, 3) for k in (3, 5, 7) for form in ("blur", "deriv")]
           + [("canny3_mono", 1, "canny", 0), ("blur5_canny3_mono", 1, "chain", 5)])


def child(name, ch, form, ks, n, steps):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from cudacam_amd import api, synth
    distinct = 8
    base = [synth.natural(W, H, 100 + k) for k in range(distinct)]
    if ch == 3:
        base = [np.stack([b, b[::-1].copy(), b[:, ::-1].copy()], -1) for b in base]
    reps = (n + distinct - 1) // distinct
    src = torch.from_numpy(np.stack(base)).cuda().repeat((reps,) + (1,) * (base[0].ndim))[:n].contiguous()
    row = ch * W
    px = n * W * H
    res = {"config": name, "channels": ch, "frames": n, "steps": steps, "ksize": ks}
    ctx = api.Context(W, H, ch, n, api.MODE_O)
    if form in ("blur", "deriv"):
        if form == "blur":
            dst = torch.empty_like(src)
            taps = api.gaussian_taps_q8(ks, 1.4)

            def run():
                ctx.gaussian_blur_device(src.data_ptr(), row, row * H, dst.data_ptr(), row, row * H, n, ks, taps)
        else:
            dx, dy = torch.empty(src.shape, dtype=torch.int16, device="cuda"), torch.empty(src.shape, dtype=torch.int16, device="cuda")

            def run():
                ctx.derivatives_device(src.data_ptr(), row, row * H, dx.data_ptr(), dy.data_ptr(), 2 * row, 2 * row * H, n, ks)
        ctx.set_stream(0)   # the null stream: torch's events bracket the kernel
        torch.cuda.synchronize()
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
        med = ms[len(ms) // 2]
        bpp = (2.0 if form == "blur" else 5.0) * ch
        res.update(ms_median=round(med, 4), ms_min=round(ms[0], 4), ms_max=round(ms[-1], 4), frames_per_s=round(n / (med / 1e3)),
                   bytes_per_px=bpp, frac_hbm=round(px * bpp / (med / 1e3) / HBM, 3))
    else:
        ctx.set_option(api.OPT_PIPELINE, 1)
        depth = max(1, ctx.pipeline_depth(n))
        out = [torch.empty((n, H, W), dtype=torch.uint8, device="cuda") for _ in range(depth)]
        tmp = [torch.empty_like(src) for _ in range(depth)] if form == "chain" else None
        taps = api.gaussian_taps_q8(5, 1.4)
        torch.cuda.synchronize()

        def run(k):
            d_in = src
            if form == "chain":
                d_in = tmp[k]
                ctx.gaussian_blur_device(src.data_ptr(), row, row * H, d_in.data_ptr(), row, row * H, n, 5, taps)
            ctx.canny_device(d_in.data_ptr(), row, row * H, out[k].data_ptr(), W, W * H, n, 50, 150, 3, False)
        for k in range(2):
            run(k % depth)
        ctx.sync()
        t0 = time.perf_counter()
        for s in range(steps):
            run(s % depth)
        ctx.sync()
        dt = (time.perf_counter() - t0) / steps
        res.update(form=ctx.last_run_info()[2], ms_per_step=round(dt * 1e3, 4), frames_per_s_pipelined=round(n / dt),
                   edge_density=round(float((out[0][0] > 0).float().mean()), 4))
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        name, ch, form, ks = next(c for c in CONFIGS if c[0] == a.child)
        n = a.frames if ch == 1 else a.frames // 2
        print(json.dumps(child(name, ch, form, ks, n, a.steps)), flush=True)
        return
    lines = []
    for name, ch, form, ks in CONFIGS:
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
