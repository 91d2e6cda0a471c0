"""Times the pieces of the automatic / per-frame thresholds of Mode O over the C ABI (profiles/auto_thr/README.md):

    python tools/auto_thr_bench.py hist  --content natural|noise|flat   k_hist256 alone (hc_histogram_device)
    python tools/auto_thr_bench.py run   --content ... [--table]        a Mode O run, with or without a per-frame table
    python tools/auto_thr_bench.py auto  --content ... [--rule otsu]    auto thresholds -> table -> run, end to end

1024 grey frames of 1920 x 1080 by default (8 distinct frames, repeated on the device), timed with events on the stream the
context runs on; one measurement per process; prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cudacam_amd import api, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["hist", "run", "auto"])
    ap.add_argument("--content", default="natural", choices=["natural", "noise", "flat"])
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--rule", default="median", choices=["median", "otsu"])
    ap.add_argument("--aperture", type=int, default=3, choices=[3, 5], help="HC_OPT_APERTURE of the run")
    a = ap.parse_args()
    import torch
    w, h, n = a.width, a.height, a.frames
    make = {"natural": lambda k: synth.natural(w, h, 100 + k), "noise": lambda k: synth.noise(w, h, 200 + k), "flat": lambda k: synth.flat(w, h, 128)}[a.content]
    base = torch.from_numpy(np.stack([make(k) for k in range(8)])).cuda()
    d = base.repeat((n + 7) // 8, 1, 1)[:n].contiguous()
    hist = torch.zeros((n, 256), dtype=torch.int32, device="cuda")
    thr = torch.tensor([[50 + (k % 7) * 10, 150 + (k % 5) * 20] for k in range(n)], dtype=torch.int32, device="cuda")
    out = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx = api.Context(w, h, 1, n, api.MODE_O)
    ctx.set_stream(s.cuda_stream)
    if a.aperture != 3:
        ctx.set_option(api.OPT_APERTURE, a.aperture)
    if a.what == "run" and a.table:
        ctx.frame_thresholds_device(thr.data_ptr(), n)
    rule = 1 if a.rule == "otsu" else 0   # api.AUTO_OTSU / api.AUTO_MEDIAN

    def step():
        if a.what == "hist":
            ctx.histogram_device(d.data_ptr(), w, w * h, n, hist.data_ptr())
        elif a.what == "run":
            ctx.run_device(d.data_ptr(), w, w * h, out.data_ptr(), w, w * h, n)
        else:
            ctx.auto_thresholds_device(d.data_ptr(), w, w * h, n, rule, 0.5 if rule else 0.33, thr.data_ptr())
            ctx.frame_thresholds_device(thr.data_ptr(), n)
            ctx.run_device(d.data_ptr(), w, w * h, out.data_ptr(), w, w * h, n)

    for _ in range(a.warmup):
        step()
    ctx.sync()
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
    res = {"what": a.what, "content": a.content, "frames": n, "width": w, "height": h, "table": bool(a.table), "aperture": a.aperture, "rule": a.rule if a.what == "auto" else None,
           "ms_median": round(med, 4), "ms_min": round(times[0], 4), "ms_max": round(times[-1], 4), "frames_per_s": round(n / med * 1e3, 1)}
    if a.what == "hist":
        res["read_TB_per_s"] = round(n * w * h / (med * 1e-3) / 1e12, 3)
        got = hist[:8].cpu().numpy()
        want = np.stack([np.bincount(f.reshape(-1), minlength=256) for f in base.cpu().numpy()])
        res["exact"] = bool(np.array_equal(got, want))
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
