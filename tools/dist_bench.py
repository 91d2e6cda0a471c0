"""Times hc_distance_transform_device over the C ABI (DESIGN.md 3.7k holds the recorded table; what this tool writes under
profiles/dist/ is measurement output and is not kept in the repository):

    python tools/dist_bench.py [--content natural,noise,corner,empty] [--frames 1,64] [--check] [--out DIR] [--record]
    python tools/dist_bench.py --report [--out DIR]

1920 x 1080 maps.  natural / noise: cv::Canny's maps (Mode O, canny_device, thresholds 50 / 150, aperture 3) of synth's natural
and noise frames, 4 distinct frames repeated on the device to `frames`; corner: a single feature pixel at (0, 0), the outward
search's worst case; empty: no feature pixel.  Per content and batch, the call is timed for both dist_types, with and without
d_nearest: both launches together, with events on the stream the context runs on, the median of --steps calls after --warmup.
Beside them, in the same process on the same maps, hc_connected_components_device at connectivity 8 with capacity 0: the comparable
existing entry, full frame in, a 4-byte plane out.  --check compares the first frame's squared distances with
scipy.ndimage.distance_transform_edt.  Prints one JSON line per measurement; --record appends them to DIR/dist_bench.jsonl
(default profiles/dist).  --report reads that file and writes DIR/README.md: the table, the ratios to the labelling and of the
worst case to the natural maps.  It needs no GPU."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cudacam_amd import api, synth  # noqa: E402

W, H, K = 1920, 1080, 4


def measure(a):
    import torch
    frames = [int(v) for v in a.frames.split(",")]
    nmax = max(frames + [K])
    s = torch.cuda.Stream()
    ctx = api.Context(W, H, 1, nmax, api.MODE_O)
    lines = []
    for content in a.content.split(","):
        if content in ("corner", "empty"):
            mapsk = torch.zeros((K, H, W), dtype=torch.uint8, device="cuda")
            if content == "corner":
                mapsk[:, 0, 0] = 255
        else:
            src = torch.from_numpy(synth.frames(content, W, H, K, seed=synth.SEED0 + 9000)).cuda()
            mapsk = torch.empty((K, H, W), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ctx.use_own_stream()
            ctx.canny_device(src.data_ptr(), W, W * H, mapsk.data_ptr(), W, W * H, K, 50, 150)
            ctx.sync()
        set_px = float((mapsk != 0).sum().item()) / K
        for n in frames:
            maps = mapsk.repeat((n + K - 1) // K, 1, 1)[:n].contiguous()
            dist = torch.empty((n, H, W), dtype=torch.int32, device="cuda")
            near = torch.empty((n, H, W), dtype=torch.int32, device="cuda")
            counts = torch.zeros((n,), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ctx.set_stream(s.cuda_stream)

            def dt(dist_type, nearest):
                ctx.distance_transform_device(maps.data_ptr(), W, W * H, n, api.DT_TO_NONZERO, dist_type, dist.data_ptr(), 4 * W, 4 * W * H,
                                              near.data_ptr() if nearest else None, 4 * W, 4 * W * H)

            def ccl():
                ctx.connected_components_device(maps.data_ptr(), W, W * H, n, 8, near.data_ptr(), 4 * W, 4 * W * H, counts.data_ptr())

            steps = [("dt_squared", lambda: dt(api.DT_SQUARED_I32, False)), ("dt_squared_nearest", lambda: dt(api.DT_SQUARED_I32, True)),
                     ("dt_f32", lambda: dt(api.DT_F32, False)), ("dt_f32_nearest", lambda: dt(api.DT_F32, True)), ("ccl_labels", ccl)]
            for name, step in steps:
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
                res = {"what": name, "content": content, "frames": n, "width": W, "height": H, "pixels_set_per_frame": round(set_px, 1),
                       "ms_median": round(times[len(times) // 2], 4), "ms_min": round(times[0], 4), "ms_max": round(times[-1], 4),
                       "ms_per_frame": round(times[len(times) // 2] / n, 4), "steps": a.steps}
                lines.append(json.dumps(res))
                print(lines[-1], flush=True)
            if a.check:
                import scipy.ndimage as ndi
                dt(api.DT_SQUARED_I32, True)
                ctx.sync()
                host = maps[0].cpu().numpy() != 0
                got, idx = dist[0].cpu().numpy(), near[0].cpu().numpy()
                if host.any():
                    edt = ndi.distance_transform_edt(~host)
                    yy, xx = np.mgrid[0:H, 0:W]
                    ok = np.array_equal(got, np.rint(edt * edt).astype(np.int64)) and host[idx // W, idx % W].all() \
                        and np.array_equal((xx - idx % W) ** 2 + (yy - idx // W) ** 2, got)
                else:
                    ok = bool((got == api.DT_NONE).all() and (idx == -1).all())
                lines.append(json.dumps({"what": "check", "content": content, "frames": n, "equals_scipy": bool(ok)}))
                print(lines[-1], flush=True)
            ctx.use_own_stream()
    ctx.close()
    if a.record:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "dist_bench.jsonl"), "a") as f:
            f.write("\n".join(lines) + "\n")


def report(a):
    rows = [json.loads(l) for l in open(os.path.join(a.out, "dist_bench.jsonl")) if l.strip()]
    t = {(r["content"], r["frames"], r["what"]): r for r in rows if r["what"] != "check"}
    checks = [r for r in rows if r["what"] == "check"]
    contents = sorted({k[0] for k in t}, key=("natural", "noise", "corner", "empty").index)
    batches = sorted({k[1] for k in t})
    kinds = ("dt_squared", "dt_squared_nearest", "dt_f32", "dt_f32_nearest", "ccl_labels")
    out = ["# hc_distance_transform_device: measurements", "",
           "Written by `python tools/dist_bench.py --report` from `dist_bench.jsonl`, which `python tools/dist_bench.py --record` appends to.",
           "1920 x 1080 maps on one MI355X; each figure is the median of the timed calls (events on the context's stream, both launches of",
           "a call together) in milliseconds PER FRAME, after warm-up calls of the same shape.  natural / noise: cv::Canny maps (50 / 150,",
           "aperture 3) of synth's frames; corner: one feature pixel at (0, 0); empty: none.  ccl_labels is",
           "hc_connected_components_device at connectivity 8 with capacity 0 on the same maps in the same process: full frame in, a 4-byte",
           "plane out.", "",
           "| content | set px / frame | frames | " + " | ".join(kinds) + " | squared+nearest / ccl |", "|---|---|---|" + "---|" * (len(kinds) + 1)]
    for c in contents:
        for n in batches:
            if (c, n, kinds[0]) not in t:
                continue
            v = [t[(c, n, k)]["ms_per_frame"] for k in kinds]
            out.append(f"| {c} | {t[(c, n, kinds[0])]['pixels_set_per_frame']:.0f} | {n} | " + " | ".join(f"{x:.4f}" for x in v) + f" | {v[1] / v[4]:.2f} |")
    out += ["", "## Ratios", ""]
    worst = None
    for n in batches:
        if ("natural", n, "dt_f32_nearest") in t and ("corner", n, "dt_f32_nearest") in t:
            r = t[("corner", n, "dt_f32_nearest")]["ms_per_frame"] / t[("natural", n, "dt_f32_nearest")]["ms_per_frame"]
            worst = max(worst or 0.0, r)
            out.append(f"- batch {n}: the single-pixel worst case takes {r:.1f} x the natural maps' time (float32 with nearest).")
        if ("natural", n, "dt_f32_nearest") in t and ("noise", n, "dt_f32_nearest") in t:
            r = t[("natural", n, "dt_f32_nearest")]["ms_per_frame"] / t[("noise", n, "dt_f32_nearest")]["ms_per_frame"]
            out.append(f"- batch {n}: the natural maps take {r:.1f} x the noise maps' time: the sparser the map, the longer the outward search of"
                       " k_dt_rows, which sets the time there, not the traffic.")
        for c in contents:
            if (c, n, "dt_squared_nearest") in t:
                out.append(f"- batch {n}, {c}: squared distances with nearest take {t[(c, n, 'dt_squared_nearest')]['ms_per_frame'] / t[(c, n, 'ccl_labels')]['ms_per_frame']:.2f} x the labelling.")
    px = W * H
    if ("natural", max(batches), "dt_f32_nearest") in t:
        ms = t[("natural", max(batches), "dt_f32_nearest")]["ms_per_frame"]
        out += ["", f"At batch {max(batches)} a natural map takes {ms:.4f} ms: the call moves about 25 bytes per pixel (1 read, 4 written and 4 read again by k_dt_cols, up",
                "to 4 more written on its way up, 4 read and 4 + 4 written by k_dt_rows), " + f"{25 * px / 1e6:.1f} MB per frame, which is {25 * px / (ms * 1e-3) / 1e12:.2f} TB/s (an",
                "estimate of the traffic from the shapes, not a counter)."]
    if checks:
        out += ["", "`--check`: squared distances equal to `rint(scipy.ndimage.distance_transform_edt(~feat)^2)` and every nearest index a feature pixel at", "that distance: "
                + ", ".join(f"{r['content']} x {r['frames']}: {'yes' if r['equals_scipy'] else 'NO'}" for r in checks) + "."]
    if worst is not None and worst > 20:
        out += ["", "## The fix that is not built", "",
                f"The worst case is {worst:.0f} x the natural maps, above 20 x.  A row whose columns mostly hold no dy (or far ones) makes every pixel walk",
                "outward over LDS words that cannot win.  What removes it is the lower envelope of the row's parabolas (Felzenszwalb and",
                "Huttenlocher's stack, or Meijster's scan): the columns that hold a dy are compacted first, the envelope of their parabolas",
                "is built once per row -- in bands of the row per wave, merged in LDS -- and every pixel then finds its parabola by position,",
                "O(W) per row instead of O(W x search).  The tie rule (smallest x', then smallest y') has to be restated for the envelope's",
                "breakpoints.  k_dt_rows would pick that path by the row's count of valid columns, which the ballot it already takes gives."]
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--content", default="natural,noise,corner,empty")
    ap.add_argument("--frames", default="1,64")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", action="store_true", help="compare the first frame with scipy.ndimage.distance_transform_edt")
    ap.add_argument("--record", action="store_true", help="append the results to OUT/dist_bench.jsonl")
    ap.add_argument("--report", action="store_true", help="write OUT/README.md from OUT/dist_bench.jsonl (no GPU)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dist"))
    a = ap.parse_args()
    report(a) if a.report else measure(a)


if __name__ == "__main__":
    main()
