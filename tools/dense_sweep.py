#!/usr/bin/env python3
"""k_front8's dense path: where its thresholds belong (profiles/r10_dense/).

  --sweep   for each dense_enter in --enter (dense_leave = 3/4 of it; HC_OPT_TEST_DENSE_ENTER / LEAVE): the front kernel
            alone on natural and on noise frames (no pipeline, one content every step, as bench.py --rotate 1
            --no-pipeline --kind K) and the benchmark's four-content rotation (pipelined), each --repeat times.
  --hist    per content the histogram of the count a window compares with the thresholds.  Needs a library built with
            -DF8_WQ_HIST=1 (HIPCANNY_LIB=...): every window leaves (count, path, first row) in the blur tap.  Three passes:
            dense path never (the queue path's necessary-condition count of every window), always (the dense path's exact
            count of the same windows) and automatic (the share of windows that run dense at the library's thresholds).

The batches are bench.py's: natural (seed set A), natural (seed set B), iid noise, the blend of three natural planes."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cudacam_amd import api, synth  # noqa: E402

W, H, LOW, HIGH = 1920, 1080, 10, 40
KINDS = ("natural", "natural-B", "noise", "blend")


def unique_frames(nat_per=10):
    a, b = synth.frames("natural", W, H, nat_per, seed=synth.SEED0), synth.frames("natural", W, H, nat_per, seed=synth.SEED0 + 500)
    pa, pb = a.astype(np.uint32), b.astype(np.uint32)
    pc = np.roll(pa, nat_per // 2, axis=0)[:, ::-1, :]
    return {"natural": a, "natural-B": b, "noise": synth.frames("noise", W, H, 8, seed=synth.SEED0 + 9000),
            "blend": ((7 * pa + 38 * pb + 19 * pc) >> 6).astype(np.uint8)}


def timed(torch, d_ins, B, enter, leave, pipeline, steps, warm_s=0.6):
    """-> (frames/s, mean front-kernel ms per batch of d_ins)"""
    ctx = api.Context(W, H, 1, B)
    ctx.set_option(api.OPT_PIPELINE, pipeline)
    ctx.set_thresholds(LOW, HIGH)
    ctx.set_option(api.OPT_TEST_DENSE_ENTER, enter)
    ctx.set_option(api.OPT_TEST_DENSE_LEAVE, leave)
    outs = [torch.empty((B, H, W), dtype=torch.uint8, device="cuda") for _ in range(ctx.pipeline_depth(B) if pipeline else 1)]
    n = [0]

    def step():
        ctx.run_device(d_ins[n[0] % len(d_ins)].data_ptr(), W, W * H, outs[n[0] % len(outs)].data_ptr(), W, W * H, B)
        n[0] += 1
    t = time.perf_counter()
    while time.perf_counter() - t < warm_s:
        for _ in range(4):
            step()
        ctx.sync()
    for _ in range(2 * len(d_ins) + (-n[0]) % len(d_ins)):
        step()
    ctx.sync()
    torch.cuda.synchronize()
    ctx.enable_profiling(True)
    ctx.profile_get(reset=True)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    ctx.sync()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    each = ctx.profile_front_each(steps + 8)
    ctx.close() if hasattr(ctx, "close") else None
    per = [float(np.mean(each[k::len(d_ins)])) for k in range(len(d_ins))] if len(each) == steps else [float("nan")] * len(d_ins)
    return B * steps / (t1 - t0), per


def sweep(a):
    import torch
    u = unique_frames()
    B = a.batch
    d = {}
    for k in KINDS:
        t = torch.from_numpy(u[k]).cuda()
        d[k] = t.repeat((B + t.shape[0] - 1) // t.shape[0], 1, 1)[:B].contiguous()
    print("# 1080p, %d frames per step, %d timed steps; alone = front kernel ms, no pipeline, that content every step; rotation = pipelined, four contents" % (B, a.steps))
    print("enter leave rep natural_alone_ms noise_alone_ms rotation_frames_per_s rot_natural_ms rot_naturalB_ms rot_noise_ms rot_blend_ms")
    for rep in range(a.repeat):
        for e in a.enter:
            lv = 3 * e // 4
            _, nat = timed(torch, [d["natural"]], B, e, lv, 0, a.steps)
            _, noi = timed(torch, [d["noise"]], B, e, lv, 0, a.steps)
            fps, per = timed(torch, [d[k] for k in KINDS], B, e, lv, 1, a.steps)
            print("%d %d %d %.4f %.4f %.0f %s" % (e, lv, rep, nat[0], noi[0], fps, " ".join("%.4f" % v for v in per)), flush=True)


def records(tap, run_rows):
    """the (count, dense, first output row) records of one frame's tap -> list"""
    out = []
    nch = (H + run_rows - 1) // run_rows
    for c in range(nch):
        r0 = c * run_rows
        for w in range((min(r0 + run_rows, H) - r0 + 4 + 5) // 6):
            for s in range(4):
                rec = tap[r0 + w, 8 * s: 8 * s + 8].view(np.uint32)
                assert rec[0] >> 24 == 0xA5, "no record: is this the F8_WQ_HIST build?"
                out.append((int(rec[0] & 0xFFFF), int(rec[0] >> 16) & 1, int(rec[1]) - 0x8000))
    return out


def hist(a):
    u = unique_frames()
    run_rows = 122   # what the library cuts 1080 rows into at 1024 frames per step (asked for here: the batch is smaller)
    edges = [0, 64, 128, 192, 256, 320, 384, 448, 512, 576, 640, 704, 769]
    print("# per window of 6 rows x 496 columns (768 half-lanes): the count compared with dense_enter / dense_leave; 1080p, runs of %d rows, thresholds %d / %d" % (run_rows, LOW, HIGH))
    print("# top / bottom: windows that hold output rows 0, 1 / H-2, H-1, which neither path counts; interior: all others")
    for k in KINDS:
        fr = u[k]
        got = {}
        for mode in (0, 1, -1):
            with api.Context(W, H, 1, fr.shape[0]) as ctx:
                ctx.set_thresholds(LOW, HIGH)
                ctx.set_option(api.OPT_FRONT_DENSE, mode)
                ctx.set_option(api.OPT_DEBUG_TAPS, 1)
                ctx.set_tuning(run_rows, 0)
                ctx.process(fr)
                tap = ctx.debug_tap(api.TAP_BLUR, fr.shape[0])
            got[mode] = [r for f in range(fr.shape[0]) for r in records(tap[f], run_rows)]
        q, x, auto = np.array(got[0]), np.array(got[1]), np.array(got[-1])
        assert (q[:, 2] == x[:, 2]).all() and (q[:, 1] == 0).all() and (x[:, 1] == 1).all()
        top, bot = q[:, 2] < 2, q[:, 2] + 5 >= H - 2
        print("\n%s: %d windows (%d top, %d bottom), dense at 512 / 384: %.2f %% of all windows" % (k, len(q), top.sum(), bot.sum(), 100.0 * auto[:, 1].mean()))
        print("  queue-path count minus exact count, interior windows: mean %.1f, max %d (never below: %s)" % ((q[:, 0] - x[:, 0])[~top & ~bot].mean(), (q[:, 0] - x[:, 0]).max(), bool((q[:, 0] >= x[:, 0]).all())))
        print("  share in the band 320..512 (queue-path count): interior %.2f %%, top %.2f %%, bottom %.2f %%" % tuple(100.0 * ((q[m, 0] > 320) & (q[m, 0] <= 512)).mean() for m in (~top & ~bot, top, bot)))
        print("  bin        " + " ".join("%7s" % ("%d-" % e) for e in edges[:-1]))
        for name, m in (("interior", ~top & ~bot), ("top", top), ("bottom", bot)):
            print("  %-9s q" % name + " ".join("%7d" % v for v in np.histogram(q[m, 0], edges)[0]))
            print("  %-9s x" % name + " ".join("%7d" % v for v in np.histogram(x[m, 0], edges)[0]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--hist", action="store_true")
    ap.add_argument("--enter", type=lambda s: [int(v) for v in s.split(",")], default=[192, 256, 320, 384, 448, 512])
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=2)
    a = ap.parse_args()
    if a.hist:
        hist(a)
    if a.sweep:
        sweep(a)
