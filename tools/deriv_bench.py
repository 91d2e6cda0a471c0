#!/usr/bin/env python3
"""Timing of k_deriv16 (hc_derivatives_device) beside its yardstick, k_front_o_ext on given gradients (front form 7), and of
the chained aperture-7 / Scharr Canny beside the fused aperture 5 and the fused forms of hc_canny_device.

Usage: tools/deriv_bench.py [--steps 20] [--frames 512] [--only a,b] [--out FILE]
Every configuration runs in a fresh process under `timeout`: 1080p, 512 frames per launch (3-channel: 256), `steps` timed
launches after two warm-up ones, median.
  deriv_<ksize>_<mono|bgr>   the kernel alone, between two events on the context's stream; its own bytes are C B/px of input
                             + 4 C B/px of int16 planes = 5 C B/px
  gradients_<mono|bgr>       form 7 (hc_profile_get_front_each): 4 C B/px of planes + 0.25 B/px of bit planes
  canny7_chain_<..>          hc_derivatives_device(7) + hc_run_gradients_device, pipelined, wall clock: frames/s
  scharr_chain_<..>          the same with ksize -1
  canny5_fused_<..>          HC_OPT_APERTURE 5, pipelined, wall clock: frames/s
  canny7_fused_<..>          hc_canny_device at aperture 7 (front form 8; thresholds x 16: the chain's map), pipelined, wall
                             clock: frames/s; also the front kernel's own median over `steps` plain profiled runs (front_ms_median)
  scharr_fused_<..>          hc_canny_device at aperture -1 (front form 9), likewise
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
KNAME = {3: "3", 5: "5", 7: "7", -1: "scharr"}
CONFIGS = ([(f"deriv_{KNAME[k]}_{'mono' if ch == 1 else 'bgr'}", ch, "deriv", k) for ch in (1, 3) for k in (3, 5, 7, -1)]
           + [("gradients_mono", 1, "grad", 3), ("gradients_bgr", 3, "grad", 3)]
           + [("canny7_chain_mono", 1, "chain", 7), ("canny5_fused_mono", 1, "ap5", 5),
              ("canny7_chain_bgr", 3, "chain", 7), ("canny5_fused_bgr", 3, "ap5", 5)]
           + [("canny7_fused_mono", 1, "fused", 7), ("scharr_chain_mono", 1, "chain", -1), ("scharr_fused_mono", 1, "fused", -1),
              ("canny7_fused_bgr", 3, "fused", 7), ("scharr_chain_bgr", 3, "chain", -1), ("scharr_fused_bgr", 3, "fused", -1)])


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
    if form not in ("ap5", "fused"):
        dx, dy = torch.empty(src.shape, dtype=torch.int16, device="cuda"), torch.empty(src.shape, dtype=torch.int16, device="cuda")

    def deriv(k):
        ctx.derivatives_device(src.data_ptr(), row, row * H, dx.data_ptr(), dy.data_ptr(), 2 * row, 2 * row * H, n, k)

    if form == "deriv":
        ctx.set_stream(0)   # the null stream: torch's events bracket the kernel
        torch.cuda.synchronize()
        for _ in range(2):
            deriv(ks)
        torch.cuda.synchronize()
        ms = []
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            deriv(ks)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms.sort()
        med = ms[len(ms) // 2]
        bpp = 5.0 * ch
        res.update(ms_median=round(med, 4), ms_min=round(ms[0], 4), ms_max=round(ms[-1], 4), frames_per_s=round(n / (med / 1e3)),
                   bytes_per_px=bpp, frac_hbm=round(px * bpp / (med / 1e3) / HBM, 3))
    elif form == "grad":
        ctx.set_thresholds(50, 150)
        out = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        deriv(3)
        ctx.sync()

        def run():
            ctx.run_gradients_device(dx.data_ptr(), dy.data_ptr(), 2 * row, 2 * row * H, out.data_ptr(), W, W * H, n)
        ctx.enable_profiling(1)
        for _ in range(2):
            run()
        ctx.sync()
        ctx.profile_get(reset=True)
        for _ in range(steps):
            run()
            ctx.sync()
        fe = sorted(ctx.profile_front_each())
        med = fe[len(fe) // 2]
        bpp = 4.0 * ch + 0.25
        res.update(form=ctx.last_run_info()[2], ms_median=round(med, 4), ms_min=round(fe[0], 4), ms_max=round(fe[-1], 4),
                   frames_per_s=round(n / (med / 1e3)), bytes_per_px=bpp, frac_hbm=round(px * bpp / (med / 1e3) / HBM, 3))
    else:
        if form == "ap5":
            ctx.set_thresholds(300, 900)
            ctx.set_option(api.OPT_APERTURE, 5)
        else:
            ctx.set_thresholds(150, 450)
        scale = 16.0 if ks == 7 else 1.0

        def fused(o):
            ctx.canny_device(src.data_ptr(), row, row * H, o.data_ptr(), W, W * H, n, 150 * scale, 450 * scale, ks, False)
        if form == "fused":   # the front kernel alone first: plain profiled runs
            o0 = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ctx.enable_profiling(1)
            for _ in range(2):
                fused(o0)
            ctx.sync()
            ctx.profile_get(reset=True)
            for _ in range(steps):
                fused(o0)
                ctx.sync()
            fe = sorted(ctx.profile_front_each())
            ctx.enable_profiling(0)
            bpp = ch + 0.25
            res.update(front_ms_median=round(fe[len(fe) // 2], 4), front_ms_min=round(fe[0], 4), front_ms_max=round(fe[-1], 4), bytes_per_px=bpp,
                       frac_hbm=round(px * bpp / (fe[len(fe) // 2] / 1e3) / HBM, 3))
            del o0
        ctx.set_option(api.OPT_PIPELINE, 1)
        depth = max(1, ctx.pipeline_depth(n))
        out = [torch.empty((n, H, W), dtype=torch.uint8, device="cuda") for _ in range(depth)]
        torch.cuda.synchronize()

        def run(o):
            if form == "ap5":
                ctx.run_device(src.data_ptr(), row, row * H, o.data_ptr(), W, W * H, n)
            elif form == "fused":
                fused(o)
            else:
                deriv(ks)
                ctx.run_gradients_device(dx.data_ptr(), dy.data_ptr(), 2 * row, 2 * row * H, o.data_ptr(), W, W * H, n)
        for k in range(2):
            run(out[k % depth])
        ctx.sync()
        t0 = time.perf_counter()
        for s in range(steps):
            run(out[s % depth])
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
