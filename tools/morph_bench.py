#!/usr/bin/env python3
"""Timing of k_morph8 (hc_morphology_device) beside its yardstick, k_gauss8 (hc_gaussian_blur_device) in the same session --
the same bytes, the same layout, heavier arithmetic -- and of canny_components with and without close=(RECT, 3).

Usage: tools/morph_bench.py [--steps 20] [--frames 512] [--only a,b] [--out FILE]
Every configuration runs in a fresh process under `timeout`; the script stops at the first leg that does not exit with 0.
1080p, 512 frames per launch (3-channel: 256), `steps` timed calls after two warm-up ones, the median with min and max.
  <erode|dilate|gradient|close>_<rect|ellipse>_<ksize>_<mono|bgr>   the call alone, between two events on the context's stream
  blur_<ksize>_<mono|bgr>                                           k_gauss8 alone (sigma 1.4, reflect-101), the same way
  components_64 / close_components_64                               Context.canny_components on 64 one-channel frames, wall clock
The bar: each erode / dilate RECT leg takes no longer than 1.2 x the blur leg of its ksize and channel count (`verdict` lines).
CLOSE against erode + dilate, GRADIENT against 2 x a primitive and the ELLIPSE legs are reported only."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM = 6.29e12
W, H = 1920, 1080
OPS = {"erode": 0, "dilate": 1, "close": 3, "gradient": 4}
SHAPES = {"rect": 0, "ellipse": 2}
CONFIGS = []
for _ch in (1, 3):
    for _k in (3, 5, 7):
        _tail = f"{_k}_{'mono' if _ch == 1 else 'bgr'}"
        CONFIGS.append((f"blur_{_tail}", _ch, "blur", _k, None))
        CONFIGS += [(f"{op}_{shape}_{_tail}", _ch, op, _k, shape) for shape in SHAPES for op in OPS]
CONFIGS += [("components_64", 1, "components", 0, None), ("close_components_64", 1, "components", 3, "rect")]


def child(name, ch, form, ks, shape, n, steps):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from cudacam_amd import api, synth
    res = {"config": name, "channels": ch, "steps": steps, "ksize": ks}
    if form == "components":
        n = 64
        frames = np.stack([synth.natural(W, H, 100 + k) for k in range(n)])
        ctx = api.Context(W, H, 1, n, api.MODE_O)
        close = (api.MORPH_RECT, ks) if ks else None
        ms = []
        for s in range(steps + 2):
            t0 = time.perf_counter()
            out = ctx.canny_components(frames, 50, 150, close=close)
            if s >= 2:
                ms.append((time.perf_counter() - t0) * 1e3)
        ms.sort()
        res.update(frames=n, ms_median=round(ms[len(ms) // 2], 3), ms_min=round(ms[0], 3), ms_max=round(ms[-1], 3),
                   components_mean=round(float(np.mean(out[2])) - 1, 1), note="wall clock, host copies of frames and results included")
        ctx.close()
        return res
    distinct = 8
    base = [synth.natural(W, H, 100 + k) for k in range(distinct)]
    if ch == 3:
        base = [np.stack([b, b[::-1].copy(), b[:, ::-1].copy()], -1) for b in base]
    reps = (n + distinct - 1) // distinct
    src = torch.from_numpy(np.stack(base)).cuda().repeat((reps,) + (1,) * (base[0].ndim))[:n].contiguous()
    dst = torch.empty_like(src)
    row = ch * W
    ctx = api.Context(W, H, ch, n, api.MODE_O)
    if form == "blur":
        taps = api.gaussian_taps_q8(ks, 1.4)

        def run():
            ctx.gaussian_blur_device(src.data_ptr(), row, row * H, dst.data_ptr(), row, row * H, n, ks, taps)
    else:
        spans = api.structuring_element(SHAPES[shape], ks)
        res["spans"] = spans

        def run():
            ctx.morphology_device(src.data_ptr(), row, row * H, dst.data_ptr(), row, row * H, n, ch, OPS[form], ks, spans)
    ctx.set_stream(0)   # the null stream: torch's events bracket the call
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
    bpp = 2.0 * ch   # a primitive's own bytes; the compound ops move about twice that
    res.update(frames=n, ms_median=round(med, 4), ms_min=round(ms[0], 4), ms_max=round(ms[-1], 4), frames_per_s=round(n / (med / 1e3)),
               frac_hbm_of_2c_bytes=round(n * W * H * bpp / (med / 1e3) / HBM, 3))
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "morph", "morph_bench.jsonl"))
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        name, ch, form, ks, shape = next(c for c in CONFIGS if c[0] == a.child)
        n = a.frames if ch == 1 else a.frames // 2
        print(json.dumps(child(name, ch, form, ks, shape, n, a.steps)), flush=True)
        return
    lines, med = [], {}
    for name, ch, form, ks, shape in CONFIGS:
        if a.only and name not in a.only.split(","):
            continue
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", name, "--steps", str(a.steps),
               "--frames", str(a.frames)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        res = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0 or not res:
            print(f"{name}: exit {r.returncode}\n{r.stderr[-2000:]}", file=sys.stderr, flush=True)
            sys.exit(1)   # the first non-zero status ends the session: nothing more is started on the GPU
        print(res[-1], flush=True)
        lines.append(res[-1])
        med[name] = json.loads(res[-1])["ms_median"]
        if form in ("erode", "dilate") and shape == "rect":
            yard = med.get(f"blur_{ks}_{'mono' if ch == 1 else 'bgr'}")
            if yard:
                v = json.dumps({"verdict": name, "ratio_to_blur": round(med[name] / yard, 3), "bar": 1.2, "met": med[name] <= 1.2 * yard})
                print(v, flush=True)
                lines.append(v)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
