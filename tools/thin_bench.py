#!/usr/bin/env python3
"""Timing of hc_thinning_device beside hc_morphology_device on the same maps, in the same session.

Usage: tools/thin_bench.py [--steps 20] [--frames 64] [--out FILE]
1080p, `frames` maps per call: cv::Canny maps (60, 150) of the bench's natural and noise contents, closed with 3 x 3 RECT and with
5 x 5 ELLIPSE, both methods.  Every timing is between two events on the context's stream, `steps` timed calls after two warm-up
ones, the median with min and max.  The measuring runs in one child process under `timeout`; a non-zero status ends the script.
Per case (content, element, method), one JSON line:
  iterations        min / mean / max of the iterations the frames needed (the status words of a max_iterations = 32 call)
  call_ms[m]        the whole call at max_iterations m = 1, 2, 3, 16, 32
  step_ms           (call_ms[2] - call_ms[1]) / 2: one sub-iteration launch of iteration 2, in which every frame still works
  idle_step_us      (call_ms[32] - call_ms[16]) / 32: one launch that every wave leaves on its first load (only where no frame
                    needs more than 15 iterations)
  pack_unpack_ms    call_ms[1] - 2 step_ms: k_thin_pack, k_thin_unpack and the zeroing, as a share of call_ms[16]
  dilate_ms, close_ms   hc_morphology_device DILATE / CLOSE 3 x 3 RECT on the same maps (entries older than the thinning)
The launches lie inside one entry, so these per-launch figures are differences of whole calls: they hold the gaps between the
launches and the host's enqueue rate as well as the kernels.  The derived bound: step_ms <= dilate_ms -- a step launch moves an
eighth of a byte per pixel each way, a k_morph8 launch one byte (`verdict` lines).

tools/thin_bench.py --trace [--frames 64] [--out FILE]: the kernels one by one, in a run of its own under
`rocprofv3 --kernel-trace`: ten calls per method at max_iterations 16 on the closed (3 x 3 RECT) natural maps after two warm-up
calls, and ten DILATE 3 x 3 launches.  Every dispatch is taken from the trace in order -- a call is k_thin_pack, 32 x k_thin_step,
k_thin_unpack -- and a step launch is filed by its iteration: `working` while every frame still removes pixels (iterations up
to the smallest count a frame needed), `idle` once every wave leaves on its first load (beyond the largest count + 1),
`mixed` between.  One `trace` line per method: the median, minimum and number of dispatches per kind in microseconds, the sum of a
call's kernels, and the k_morph8 launches beside them."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1920, 1080
ITER_CALLS = (1, 2, 3, 16, 32)
TRACE_CALLS = 10
THIN_METHOD_IDS = {"zhangsuen": 0, "guohall": 1}


def child(n, steps):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from cudacam_amd import api, synth
    fs = W * H
    ctx = api.Context(W, H, 1, n, api.MODE_O)
    distinct = min(8, n)
    reps = (n + distinct - 1) // distinct

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
        return ms[len(ms) // 2], ms[0], ms[-1]

    for content in ("natural", "noise"):
        frames = synth.frames(content, W, H, distinct, seed=synth.SEED0 + 77)
        edges = ctx.canny(frames, 60, 150)
        for shape_name, shape, ks in (("rect3", api.MORPH_RECT, 3), ("ellipse5", api.MORPH_ELLIPSE, 5)):
            closed = ctx.morphology(edges, api.MORPH_CLOSE, shape, ks)
            src = torch.from_numpy(closed).cuda().repeat((reps, 1, 1))[:n].contiguous()
            dst = torch.empty_like(src)
            status = torch.empty((n, 2), dtype=torch.int32, device="cuda")
            ctx.set_stream(0)   # the null stream: torch's events bracket the call
            torch.cuda.synchronize()
            r3 = api.structuring_element(api.MORPH_RECT, 3)
            morph = {}
            for op_name, op in (("dilate", api.MORPH_DILATE), ("close", api.MORPH_CLOSE)):
                morph[op_name] = timed(lambda: ctx.morphology_device(src.data_ptr(), W, fs, dst.data_ptr(), W, fs, n, 1, op, 3, r3))
            for method_name, method in api.THIN_METHODS.items():
                ctx.thinning_device(src.data_ptr(), W, fs, dst.data_ptr(), W, fs, n, method, 32, status.data_ptr())
                torch.cuda.synchronize()
                st = status.cpu().numpy().view(np.uint32)
                its = st[:, 0]
                call = {m: timed(lambda: ctx.thinning_device(src.data_ptr(), W, fs, dst.data_ptr(), W, fs, n, method, m, status.data_ptr())) for m in ITER_CALLS}
                step = (call[2][0] - call[1][0]) / 2
                res = {"case": f"{content}_{shape_name}_{method_name}", "frames": n, "steps": steps, "density": round(float((closed != 0).mean()), 4),
                       "iterations": [int(its.min()), round(float(its.mean()), 2), int(its.max())], "converged": int(st[:, 1].min()),
                       "call_ms": {str(m): [round(v, 4) for v in call[m]] for m in ITER_CALLS}, "step_ms": round(step, 4),
                       "pack_unpack_ms": round(call[1][0] - 2 * step, 4), "pack_unpack_share_of_16": round((call[1][0] - 2 * step) / call[16][0], 3),
                       "dilate_ms": [round(v, 4) for v in morph["dilate"]], "close_ms": [round(v, 4) for v in morph["close"]],
                       "call16_over_close": round(call[16][0] / morph["close"][0], 3), "step_over_dilate": round(step / morph["dilate"][0], 3)}
                if its.max() <= 15:
                    res["idle_step_us"] = round((call[32][0] - call[16][0]) / 32 * 1e3, 2)
                print(json.dumps(res), flush=True)
                print(json.dumps({"verdict": res["case"], "step_over_dilate": res["step_over_dilate"], "bar": 1.0, "met": step <= morph["dilate"][0]}), flush=True)
            ctx.use_own_stream()
    ctx.close()


def trace_child(n):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from cudacam_amd import api, synth
    fs = W * H
    ctx = api.Context(W, H, 1, n, api.MODE_O)
    distinct = min(8, n)
    frames = synth.frames("natural", W, H, distinct, seed=synth.SEED0 + 77)
    closed = ctx.morphology(ctx.canny(frames, 60, 150), api.MORPH_CLOSE, api.MORPH_RECT, 3)
    src = torch.from_numpy(closed).cuda().repeat(((n + distinct - 1) // distinct, 1, 1))[:n].contiguous()
    dst = torch.empty_like(src)
    status = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    its = {}
    for name, method in api.THIN_METHODS.items():
        for _ in range(2 + TRACE_CALLS):
            ctx.thinning_device(src.data_ptr(), W, fs, dst.data_ptr(), W, fs, n, method, 16, status.data_ptr())
            ctx.sync()
        st = status.cpu().numpy().view(np.uint32)
        its[name] = [int(st[:, 0].min()), int(st[:, 0].max())]
    r3 = api.structuring_element(api.MORPH_RECT, 3)
    for _ in range(2 + TRACE_CALLS):
        ctx.morphology_device(src.data_ptr(), W, fs, dst.data_ptr(), W, fs, n, 1, api.MORPH_DILATE, 3, r3)
        ctx.sync()
    ctx.close()
    print(json.dumps({"trace_iterations": its, "frames": n}), flush=True)


def trace_lines(csv_path, its, n):
    """The `trace` lines from a rocprofv3 kernel-trace CSV (rows with Kernel_Name, Start_Timestamp, End_Timestamp in ns)."""
    import csv
    import re
    import statistics
    rows = sorted(csv.DictReader(open(csv_path)), key=lambda r: int(r["Start_Timestamp"]))
    calls, morph, cur = [], [], None
    for r in rows:
        name, us = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        step = re.search(r"k_thin_step<\s*(\d)\s*,\s*(\d)\s*>", name) or re.search(r"k_thin_stepILi(\d)ELi(\d)E", name)
        if "k_thin_pack" in name:
            cur = {"pack": us, "steps": [], "method": None}
        elif step and cur is not None:
            cur["method"] = int(step.group(1))
            cur["steps"].append(us)
        elif "k_thin_unpack" in name and cur is not None:
            cur["unpack"] = us
            calls.append(cur)
            cur = None
        elif "k_morph8" in name:
            morph.append(us)
    out = []
    dil = morph[-TRACE_CALLS:]   # (the launches before them are the closing of the maps and the warm-up)
    for mname, (imin, imax) in its.items():
        mine = [c for c in calls if c["method"] == THIN_METHOD_IDS[mname] and len(c["steps"]) == 32][-TRACE_CALLS:]
        if not mine:
            continue
        kinds = {"pack": [c["pack"] for c in mine], "unpack": [c["unpack"] for c in mine], "working": [], "mixed": [], "idle": []}
        for c in mine:
            for j, us in enumerate(c["steps"]):
                it = j // 2 + 1
                kinds["working" if it <= imin else "idle" if it > imax + 1 else "mixed"].append(us)
        res = {"trace": f"natural_rect3_{mname}", "frames": n, "calls": len(mine), "iterations_min_max": [imin, imax],
               "kernels_per_call_us": round(statistics.median(c["pack"] + c["unpack"] + sum(c["steps"]) for c in mine), 2)}
        for k, v in kinds.items():
            if v:
                res[k + "_us"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "dispatches": len(v)}
        if dil:
            res["dilate_us"] = {"median": round(statistics.median(dil), 2), "min": round(min(dil), 2), "dispatches": len(dil)}
        out.append(json.dumps(res))
    return out


def trace(a):
    import glob
    import shutil
    import tempfile
    out_dir = os.path.dirname(os.path.abspath(a.out)) if a.out else tempfile.gettempdir()
    os.makedirs(out_dir, exist_ok=True)
    d = os.path.join(out_dir, "thin_trace_tmp")
    shutil.rmtree(d, ignore_errors=True)
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--trace-child",
           "--frames", str(a.frames)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=tempfile.gettempdir())
    info = [l for l in r.stdout.splitlines() if l.startswith('{"trace_iterations"')]
    if r.returncode != 0 or not info:
        print(f"exit {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}", file=sys.stderr, flush=True)
        sys.exit(1)   # nothing more is started on the GPU
    j = json.loads(info[-1])
    files = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
    if not files:
        sys.exit("no kernel trace was written")
    lines = trace_lines(max(files, key=os.path.getsize), j["trace_iterations"], j["frames"])
    shutil.rmtree(d, ignore_errors=True)
    print("\n".join(lines), flush=True)
    if a.out and lines:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thinning", "thin_bench.jsonl"))
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
            a.out = os.path.join(ROOT, "profiles", "thinning", "thin_trace.jsonl")
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
