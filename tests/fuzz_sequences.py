#!/usr/bin/env python3
"""Randomised run SEQUENCES on the GPU box: one context per case, 8-20 runs whose content, batch size, entry point and
options change from run to run, every map of every run compared with the oracle.

The host side of the library schedules a run by what the earlier runs of its context observed (launches queued, worklists
or a workgroup per tile, grids sized from the last run's lists, tile height, pipeline slots); a wrong prediction may cost
time, never a pixel.  tests/fuzz_parity.py opens a fresh context per case, so it never shows the library a history that
disagrees with the content.  This tool does nothing else.

Usage: tests/fuzz_sequences.py [cases] [seed]
       tests/fuzz_sequences.py --case-seed N     (one case alone: the case_seed of a mismatch line)
Exit status 1 on any mismatch; one line per mismatch with everything needed to replay it (tool seed, case index, the
case's own seed, index of the failing run).  The final line counts cases, runs, maps compared, refused calls, mismatches.

What the random cases do not reach: their batches stay at 24 frames or fewer on the wide geometries, so no run has the
2048 tiles from which a grid sized by the previous run's lists is smaller than the tile count -- lists longer than such a
grid are covered by the scripted wide-frame and big-batch sequences of tests/test_gpu_history.py only.

The module is also the runner of the scripted sequences in tests/test_gpu_history.py (class Sequence)."""
import ctypes as C
import os
import sys
import time
from multiprocessing.pool import ThreadPool

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # repo root
from cudacam_amd import api, synth


# ---- content ----------------------------------------------------------------------------------------------------------
# (synth.serpentine does not chain in Mode R at 10 / 40: between its strong head and its weak band non-maximum suppression
#  leaves a gap, and the hysteresis has nothing to follow -- oracle: 60 edge pixels, the head alone.  The two generators
#  below grade the head down into the band, as the `line` frame of test_download_begin_end does; their weak edges are
#  reached from the head only, one tile-boundary crossing per launch.)
def wobble(w, h, yb, amp_rows, period, level=20, head=120):
    """A step edge along a triangle wave around row yb: weak along its whole length, strong only at its left end.  With yb
    on a tile boundary the edge crosses it twice per period, and each crossing costs the hysteresis one launch."""
    x = np.arange(w)
    ph = (x % period) / period
    tri = np.where(ph < 0.5, 4 * ph - 1, 3 - 4 * ph)
    f = np.clip(np.round(yb + amp_rows * tri).astype(int), 2, max(2, h - 3))
    img = np.where(np.arange(h)[:, None] >= f[None, :], level, 0).astype(np.int32)
    n = min(20, w // 4)
    for c in range(n):
        col = img[:, c]
        col[col > 0] = head - (head - level) * c // max(n, 1)
    return img.astype(np.uint8)


def vchain(w, h, level=20, head=120):
    """A weak vertical bar down the whole frame with a graded strong head in its first rows: crosses every row tile once."""
    x0 = w // 8
    x1 = max(x0 + 1, min(w - 2, x0 + 40))
    img = np.zeros((h, w), np.uint8)
    img[:, x0:x1] = level
    for r in range(min(20, h // 2)):
        img[r, x0:x1] = head - (head - level) * r // 20
    return img


def sparse_edges(w, h, seed):
    """A few long high-contrast lines: strong edges that need no propagation, very few tiles with late work."""
    img = np.zeros((h, w), np.uint8)
    r = np.random.default_rng(seed)
    for _ in range(3):
        y = int(r.integers(0, h))
        img[y:y + 3, :] = 200
    x = int(r.integers(0, w))
    img[:, x:x + 3] = 200
    return img


KINDS = ("zero", "flat", "noise", "natural", "wobble", "vchain", "sparse")


def make_frame(kind, w, h, seed=1):
    if kind == "zero":
        return np.zeros((h, w), np.uint8)
    if kind == "flat":
        return synth.flat(w, h, 90)
    if kind == "noise":
        return synth.noise(w, h, seed)
    if kind == "natural":
        return synth.natural(w, h, seed)
    if kind == "wobble":   # around the first boundary of 64-row tiles (also one of 128-row tiles when the frame has one)
        yb = 128 if h > 160 else 64 if h > 68 else h // 2
        return wobble(w, h, yb, max(1, min(20, h - yb - 3, yb - 3)), max(8, w // 15))
    if kind == "vchain":
        return vchain(w, h)
    if kind == "sparse":
        return sparse_edges(w, h, seed)
    raise ValueError(kind)


def to_channels(f, ch):
    if ch == 1:
        return f
    return np.stack([np.roll(f, 5 * c, axis=0) ^ np.uint8(17 * c) for c in range(3)], axis=-1)


def thr_maps(w, h, seed=3):
    """Tri-state maps for hc_hysteresis_device: empty, a 1-px serpentine from one seed, clutter, all candidates + one seed."""
    one = np.full((h, w), 128, np.uint8)
    one[h - 1, w - 1] = 255
    serp = synth.thresh_map_serpentine(w, h) if w >= 3 and h >= 3 else one.copy()
    return [np.zeros((h, w), np.uint8), serp, synth.thresh_map_random(w, h, seed, 0.40, 0.002), one]


class Mismatch(AssertionError):
    pass


class Sequence:
    """One context, a pool of distinct frames, and runs that pick frames from the pool by index.  Every map of every run is
    compared with the oracle's (memoised per frame and setting, compared on the device: torch.equal over the whole batch).
    Runs that are not synchronised stay in flight, each in an output buffer of its own, at most `nbuf` of them; the burst is
    completed and checked before a buffer is used again; every output buffer is overwritten with 7 before a run is queued
    into it, so equal maps are this run's.  `log` holds what the diagnostics said about a run -- but only for runs whose
    completion the sequence saw ONE AT A TIME (hc_last_* describe the most recent completed run alone): runs that had others
    in flight are compared like all the rest, but their schedules are not in the log, and assertions on the log say nothing
    about them."""

    def __init__(self, O, w, h, pool, ch=1, max_batch=4, mode="R", per_channel=False, nbuf=2, thr_pool=None, threads=16):
        import torch
        self.torch, self.O = torch, O
        self.w, self.h, self.ch, self.max_batch, self.mode, self.pc = w, h, ch, max_batch, mode, bool(per_channel)
        self.maps = 3 if self.pc else 1
        self.pool = [np.ascontiguousarray(to_channels(f, ch)) for f in pool]
        self.thr_pool = thr_pool or []
        self.ip = (w + 7) // 8 * 8 * ch       # input pitch: whole 8-pixel groups
        self.op = (w + 3) // 4 * 4
        self.tp = (w + 3) // 4 * 4
        self.dev = torch.device("cuda", 0)
        buf = np.zeros((len(self.pool), h, self.ip), np.uint8)
        for k, f in enumerate(self.pool):
            buf[k, :, :w * ch] = f.reshape(h, w * ch)
        self.d_pool = torch.from_numpy(buf).to(self.dev)
        if self.thr_pool:
            tb = np.zeros((len(self.thr_pool), h, self.tp), np.uint8)
            tb[:, :, :w] = np.stack(self.thr_pool)
            self.d_thr = torch.from_numpy(tb).to(self.dev)
        self.nbuf = nbuf
        self.d_out = [torch.zeros((max_batch * self.maps, h, self.op), dtype=torch.uint8, device=self.dev) for _ in range(nbuf)]
        self.ctx = api.Context(w, h, ch, max_batch, api.MODE_R if mode == "R" else api.MODE_O)
        if self.pc:
            self.ctx.set_option(api.OPT_PER_CHANNEL, 1)
        self.lo, self.hi = self.ctx.get_thresholds()
        self.sat = self.l2 = 0
        self.want = {}        # setting -> (device tensor [pool][maps][h][w], set of filled indices)
        self.pending = []     # (run index, buffer index, index tensor, setting or "thr", n, keep-alive)
        self.next_buf = 0
        self.run_no = 0
        self.maps_compared = 0
        self.log = []
        self.tp_threads = ThreadPool(threads)
        self.hout = None
        self.null_stream_load = None   # callable: queues work on torch's default stream just before hc_run_device (device() only)

    def close(self):
        try:
            self.ctx.close()
        finally:
            self.tp_threads.close()
            if self.hout:
                self.ctx.lib.hc_host_free(C.c_void_p(self.hout))
                self.hout = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- settings --
    def thresholds(self, lo, hi):
        self.ctx.set_thresholds(lo, hi)   # (takes effect with the next run; runs in flight keep theirs)
        self.lo, self.hi = self.ctx.get_thresholds()

    def option(self, opt, value):
        self.ctx.set_option(opt, value)   # (completes the runs in flight: the burst can be checked)
        if opt == api.OPT_NMS_SATURATE:
            self.sat = int(bool(value))
        if opt == api.OPT_L2_GRADIENT:
            self.l2 = int(bool(value))
        self.flush(record=False)

    # -- the oracle, memoised --
    def _oracle_one(self, key):
        kind, i, lo, hi, sat, l2 = key
        if kind == "thr":
            return self.O.hysteresis(self.thr_pool[i])[None]
        f = self.pool[i]
        if self.mode == "O":
            return self.O.canny_o(f, lo, hi, l2gradient=bool(l2))[None]
        if self.pc:
            return np.stack([self.O.canny_r(np.ascontiguousarray(f[:, :, c]), lo, hi, saturate=bool(sat)) for c in range(3)])
        return self.O.canny_r(f, lo, hi, saturate=bool(sat))[None]

    def _want(self, kind, idx):
        setting = ("thr",) if kind == "thr" else ("c", self.lo, self.hi, self.sat, self.l2)
        npool = len(self.thr_pool) if kind == "thr" else len(self.pool)
        nm = 1 if kind == "thr" else self.maps
        if setting not in self.want:
            self.want[setting] = (self.torch.zeros((npool, nm, self.h, self.w), dtype=self.torch.uint8, device=self.dev), set())
        t, have = self.want[setting]
        miss = sorted(set(int(i) for i in idx) - have)
        if miss:
            keys = [("thr", i, 0, 0, 0, 0) if kind == "thr" else ("c", i, self.lo, self.hi, self.sat, self.l2) for i in miss]
            for i, m in zip(miss, self.tp_threads.map(self._oracle_one, keys)):
                t[i] = self.torch.from_numpy(np.ascontiguousarray(m)).to(self.dev)
                have.add(i)
        return setting

    def _compare(self, got, setting, idx_t, n, run, what):
        """got: device tensor [n * maps][h][>= w]"""
        t = self.want[setting][0]
        nm = t.shape[1]
        want = t.index_select(0, idx_t).reshape(n * nm, self.h, self.w)
        g = got[: n * nm, :, : self.w]
        self.maps_compared += n * nm
        if self.torch.equal(g, want):
            return
        bad = (g != want).reshape(n * nm, -1).sum(dim=1).cpu().numpy()
        first, last = int(np.flatnonzero(bad)[0]), int(np.flatnonzero(bad)[-1])
        pos = self.torch.nonzero(g[first] != want[first])[0].tolist()
        try:   # (the runs are complete here) what the diagnostics say about the last one: ring size, schedule
            state = f"; last completed run: slots {self.ctx.pipeline_slots_in_use()} info {self.ctx.hysteresis_info()} schedule {self.ctx.hysteresis_schedule()}"
        except api.HipCannyError as e:
            state = f"; diagnostics unavailable: {e}"
        raise Mismatch(f"run {run} ({what}): {int((bad > 0).sum())} of {n * nm} maps differ (maps {first} .. {last}), first map {first} (pool frame {int(idx_t[first // nm])}): "
                       f"{int(bad[first])} px, first at {pos}: hip {int(g[first][pos[0], pos[1]])} oracle {int(want[first][pos[0], pos[1]])}" + state)

    # -- completion --
    def flush(self, record=True):
        """Completes everything in flight and checks it.  record: the diagnostics describe the last run completed -- they are
        logged when exactly one run was in flight."""
        if not self.pending:
            return
        self.ctx.sync()
        one = len(self.pending) == 1
        pend, self.pending = self.pending, []
        if record and one:
            self._record(pend[0][0], pend[0][6])
        for run, b, idx_t, setting, n, keep, what in pend:
            self._compare(self.d_out[b], setting, idx_t, n, run, what)

    def _record(self, run, what):
        work, cont = self.ctx.hysteresis_info()
        s = self.ctx.hysteresis_schedule()
        s.update(run=run, what=what, work=work, cont=cont, slots=self.ctx.pipeline_slots_in_use())
        self.log.append(s)

    # -- runs --
    def _idx(self, idx):
        return self.torch.tensor([int(i) for i in idx], dtype=self.torch.long, device=self.dev)

    def _take_buffer(self):
        b = self.next_buf
        if any(p[1] == b for p in self.pending):
            self.flush()
        self.next_buf = (b + 1) % self.nbuf
        return b

    def device(self, idx, sync=True):
        """hc_run_device on frames idx of the pool, into the next output buffer of the ring."""
        run, self.run_no = self.run_no, self.run_no + 1
        n = len(idx)
        setting = self._want("c", idx)
        b = self._take_buffer()
        idx_t = self._idx(idx)
        d_in = self.d_pool.index_select(0, idx_t)
        self.d_out[b].fill_(7)   # whatever an earlier run left here (perhaps the right maps for this very content) is gone
        self.torch.cuda.current_stream().synchronize()   # the context stream does not wait for torch's
        if self.null_stream_load is not None:   # work of the caller's own on the null stream (torch's default), in flight while the run is queued
            self.null_stream_load()
        self.ctx.run_device(d_in.data_ptr(), self.ip, self.ip * self.h, self.d_out[b].data_ptr(), self.op, self.op * self.h, n)
        self.pending.append((run, b, idx_t, setting, n, d_in, f"run_device n={n}"))
        if sync:
            self.flush()
        return run

    def hyst(self, idx, sync=True):
        """hc_hysteresis_device on maps idx of the threshold-map pool."""
        run, self.run_no = self.run_no, self.run_no + 1
        n = len(idx)
        setting = self._want("thr", idx)
        b = self._take_buffer()
        idx_t = self._idx(idx)
        d_in = self.d_thr.index_select(0, idx_t)
        self.d_out[b].fill_(7)
        self.torch.cuda.current_stream().synchronize()
        self.ctx.hysteresis_device(d_in.data_ptr(), self.tp, self.tp * self.h, self.d_out[b].data_ptr(), self.op, self.op * self.h, n)
        self.pending.append((run, b, idx_t, setting, n, d_in, f"hysteresis_device n={n}"))
        if sync:
            self.flush()
        return run

    def _host_batch(self, idx):
        return np.stack([self.pool[int(i)] for i in idx])

    def process(self, idx):
        """hc_upload / hc_run / hc_download through the internal buffers (synchronous)."""
        self.flush()   # (hc_upload completes the runs in flight anyway; check them first so that the log stays in order)
        run, self.run_no = self.run_no, self.run_no + 1
        n = len(idx)
        setting = self._want("c", idx)
        got = self.ctx.process(self._host_batch(idx))
        self._record(run, f"process n={n}")
        self._compare(self.torch.from_numpy(got).to(self.dev), setting, self._idx(idx), n, run, f"process n={n}")
        return run

    def download_split(self, idx, between=None):
        """hc_upload / hc_run / hc_download_begin ... `between` (another call on the context) ... hc_download_end."""
        self.flush()
        run, self.run_no = self.run_no, self.run_no + 1
        n = len(idx)
        nm = n * self.maps
        setting = self._want("c", idx)
        lib = self.ctx.lib
        if not self.hout:
            self.hout = lib.hc_host_alloc(self.max_batch * self.maps * self.w * self.h)
        host = np.ctypeslib.as_array((C.c_uint8 * (nm * self.w * self.h)).from_address(self.hout)).reshape(nm, self.h, self.w)
        host[:] = 7
        self.ctx.upload(self._host_batch(idx))
        self.ctx.run(api.CannyStage.HYSTER, n)
        api._ck(lib.hc_download_begin(self.ctx.handle, C.c_void_p(self.hout), self.w, self.w * self.h, nm))
        try:
            if between is not None:
                between()
        finally:
            api._ck(lib.hc_download_end(self.ctx.handle))
        got = self.torch.from_numpy(host.copy()).to(self.dev)
        del host   # (a view of pinned memory that close() frees: it must not live on in the traceback of a mismatch)
        self._compare(got, setting, self._idx(idx), n, run, f"download_begin/end n={n}")
        self.flush()
        return run

    def refused(self, call, message):
        """A call the header documents as refused: HC_E_ARG (-1) and the message."""
        try:
            call()
        except api.HipCannyError as e:
            assert "error -1:" in str(e) and message in str(e), f"refused, but not as documented: {e}"
            return
        raise AssertionError(f"the library accepted a call it documents as refused ({message})")


# ---- the randomised tool ----------------------------------------------------------------------------------------------
def geometry(rng):
    """(w, h, max_batch): the classes of the scripted sequences plus the small sizes of fuzz_parity."""
    c = rng.random()
    if c < 0.30:
        return int(rng.integers(1, 600)), int(rng.integers(1, 200)), int(rng.integers(1, 5))
    if c < 0.55:
        return int(rng.choice([300, 640, 1000])), int(rng.choice([200, 480, 1400])), int(rng.integers(1, 5))   # one panel, the looping launch
    if c < 0.65:
        return 1920, 1080, int(rng.choice([2, 6]))
    if c < 0.85:
        return int(rng.choice([2100, 4500])), int(rng.choice([150, 300])), int(rng.choice([3, 8, 24]))   # several panels
    return int(rng.choice([6000, 8184])), 70, int(rng.choice([4, 16]))


def one_case(O, case_seed, stats):
    rng = np.random.default_rng(case_seed)
    w, h, mb = geometry(rng)
    mode = "R" if rng.random() < 0.7 else "O"
    ch = 3 if rng.random() < 0.25 else 1
    pc = ch == 3 and mode == "R" and rng.random() < 0.5
    kinds = list(rng.choice(KINDS, 5, replace=True)) + ["zero"]
    pool = [make_frame(k, w, h, int(rng.integers(1, 1 << 20))) for k in kinds]
    nbuf = int(rng.choice([2, 4]))
    nruns = int(rng.integers(8, 21))
    with Sequence(O, w, h, pool, ch=ch, max_batch=mb, mode=mode, per_channel=pc, nbuf=nbuf, thr_pool=thr_maps(w, h, int(rng.integers(1, 99)))) as s:
        piped = False
        for r in range(nruns):
            stats["run"] = s.run_no
            n = int(rng.integers(1, mb + 1))
            idx = [int(v) for v in rng.integers(0, len(pool), n)]   # the kind of every frame on its own
            if rng.random() < 0.33:
                hi_max = 256 if mode == "R" else 600
                s.thresholds(*sorted(int(v) for v in rng.integers(0, hi_max, 2)))
            if rng.random() < 0.25:
                want_piped = bool(rng.integers(0, 2))
                if want_piped != piped:
                    s.option(api.OPT_PIPELINE, int(want_piped))
                    piped = want_piped
            if rng.random() < 0.3:
                if mode == "R":
                    opt, val = [(api.OPT_NMS_SATURATE, int(rng.integers(0, 2))), (api.OPT_FRONT_MX, int(rng.integers(0, 2))), (api.OPT_FRONT_HALF, int(rng.choice([-1, 0, 1]))),
                                (api.OPT_FRONT_WPB, int(rng.choice([-1, 1, 4]))), (api.OPT_FRONT_DENSE, int(rng.choice([-1, 0, 1])))][int(rng.integers(0, 5))]
                else:
                    opt, val = api.OPT_L2_GRADIENT, int(rng.integers(0, 2))   # (aperture 5 has an oracle of its own, tests/canny_o_ext_ref.py: not part of these sequences)
                s.option(opt, val)
            if rng.random() < 0.04:   # documented refusal: more frames than the context was created for
                s.refused(lambda: s.ctx.run_device(s.d_pool.data_ptr(), s.ip, s.ip * h, s.d_out[0].data_ptr(), s.op, s.op * h, mb + 1), "nframes out of range")
                stats["refused"] += 1
            e = rng.random()
            sync = bool(rng.random() < 0.5)
            if e < 0.45:
                s.device(idx, sync=sync)
            elif e < 0.65:
                s.process(idx)
            elif e < 0.85:
                s.hyst([int(v) for v in rng.integers(0, len(s.thr_pool), n)], sync=sync)
            else:
                other = [int(v) for v in rng.integers(0, len(pool), n)]
                s.download_split(idx, between=(lambda: s.device(other, sync=False)) if rng.random() < 0.6 else None)
        s.flush()
        stats["run"] = s.run_no
        stats["runs"] += s.run_no
        stats["maps"] += s.maps_compared
    return f"{w}x{h} ch {ch} mode {mode} pc {int(pc)} max_batch {mb} nbuf {nbuf} kinds {','.join(kinds)}"


def main(argv):
    api.preload_hip_runtime()
    from oracle import oracle as O
    O.build()
    if len(argv) > 2 and argv[1] == "--case-seed":
        stats = {"runs": 0, "maps": 0, "refused": 0, "run": 0}
        try:
            print("case:", one_case(O, int(argv[2]), stats))
        except Mismatch as e:
            print(f"MISMATCH case_seed {argv[2]} failing {e}")
            return 1
        print(f"sequences: 1 case, {stats['runs']} runs, {stats['maps']} maps compared, {stats['refused']} refused calls (as documented), 0 mismatches")
        return 0
    cases = int(argv[1]) if len(argv) > 1 else 100
    seed = int(argv[2]) if len(argv) > 2 else 12345
    top = np.random.default_rng(seed)
    stats = {"runs": 0, "maps": 0, "refused": 0, "run": 0}
    bad = 0
    t0 = time.time()
    for i in range(cases):
        case_seed = int(top.integers(1, 1 << 62))
        try:
            one_case(O, case_seed, stats)
        except Mismatch as e:
            bad += 1
            print(f"MISMATCH tool seed {seed} case {i} case_seed {case_seed} failing {e}", flush=True)
        except api.HipCannyError as e:   # an error return ends the tool: nothing further is started on the device
            print(f"ERROR tool seed {seed} case {i} case_seed {case_seed} run {stats['run']}: {e}", flush=True)
            print(f"sequences: stopped after {i} of {cases} cases", flush=True)
            return 2
    print(f"sequences: seed {seed}, {cases} cases, {stats['runs']} runs, {stats['maps']} maps compared, {stats['refused']} refused calls (as documented), "
          f"{bad} mismatches, {time.time() - t0:.1f} s")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
