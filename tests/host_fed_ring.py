"""The host-fed ring over the C ABI, written once for the tests: `depth` contexts, each with its own hostIn / hostOut, fed
hc_upload -> hc_run -> hc_download_begin and completed (hc_download_end) oldest first -- the Python twin of
cvp::io::FrameStreamer (include/cvp/frameIO.hpp), as bench.py's host-fed leg writes it inline.  Unlike that one every batch
has its own content, hostOut is poisoned before every hc_download_begin, each completed batch comes back as a copy of the
WHOLE hostOut with its batch index, and the host strides, the mode and the options are parameters.

schedule() and RingOrder are pure (tests/test_host_fed_ring_cpu.py); Ring and the blocker of the ordering tests need the MI355X."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:   # (tests/conftest.py does the same; the two-thread case runs this file in a fresh process)
    sys.path.insert(0, ROOT)

from cudacam_amd import api, synth   # noqa: E402

POISON = 0x4D
KINDS = ("natural", "noise", "steps", "flat")
NCONTENTS = len(KINDS)   # contents 0 .. 3: frame f of content c is of kind (c + f) % 4, so two contents differ in every frame


# ---- the order of a ring (pure) -----------------------------------------------------------------------------------------
class RingOrder:
    """Which slot a batch takes and which batch a commit completes: batch i goes to slot i % depth; once every slot is busy
    the commit that queued batch i completes the oldest one in flight, so that the next commit finds its slot free."""

    def __init__(self, depth):
        self.depth = int(depth)
        self.inflight = []   # batch indices, oldest first
        self.next = 0

    def commit(self):
        """(batch index, slot, batch to complete now or None)"""
        i = self.next
        self.next += 1
        self.inflight.append(i)
        done = self.inflight.pop(0) if len(self.inflight) >= self.depth else None
        return i, i % self.depth, done

    def flush(self):
        """the batches still in flight, oldest first"""
        rest, self.inflight = self.inflight, []
        return rest


def schedule(nbatches, depth, max_batch, seed):
    """What a ring of `depth` slots is fed: {"batches": [(content, nframes)], "events": [("queue" | "complete", batch,
    slot)], "completes": [batch]}.  Frame counts run over 1 .. max_batch -- every count occurs once nbatches >= max_batch --
    and the last batch is ragged (fewer than max_batch frames, where max_batch > 1); the content of a batch differs from
    that of the batch before it on the same slot and from that of the batch before it in the stream."""
    rng = np.random.default_rng(seed)
    counts = [int(v) for v in rng.integers(1, max_batch + 1, nbatches)]
    for k in range(min(max_batch, nbatches)):   # every count at least once, then in a random order
        counts[k] = k + 1
    counts = [counts[int(k)] for k in rng.permutation(nbatches)]
    if max_batch > 1 and counts[-1] == max_batch:   # the ragged end: change places with a shorter batch, or shorten
        short = [k for k in range(nbatches - 1) if counts[k] < max_batch]
        if short:
            counts[-1], counts[short[0]] = counts[short[0]], counts[-1]
        else:
            counts[-1] = max_batch - 1
    contents = []
    for i in range(nbatches):
        banned = {contents[i - depth] if i >= depth else -1, contents[i - 1] if i >= 1 else -1}
        contents.append(int(rng.choice([c for c in range(NCONTENTS) if c not in banned])))
    ring, events, completes = RingOrder(depth), [], []
    for _ in range(nbatches):
        i, slot, done = ring.commit()
        events.append(("queue", i, slot))
        if done is not None:
            events.append(("complete", done, done % depth))
            completes.append(done)
    for done in ring.flush():
        events.append(("complete", done, done % depth))
        completes.append(done)
    return {"batches": list(zip(contents, counts)), "events": events, "completes": completes}


# ---- content ------------------------------------------------------------------------------------------------------------
def _plane(kind, w, h, seed):
    if kind == "natural":
        return synth.natural(w, h, seed)
    if kind == "noise":
        return synth.noise(w, h, seed)
    if kind == "steps":
        return synth.steps(w, h, 120 + seed % 100, ("vertical", "horizontal", "diagonal")[seed % 3], base=20)
    return synth.flat(w, h, 30 + seed % 200)


def content_frames(content, w, h, ch, n, salt=0):
    """The n frames of a content: (n, h, w) u8, or (n, h, w, 3) B, G, R with a plane of its own per channel."""
    out = []
    for f in range(n):
        kind, seed = KINDS[(content + f) % len(KINDS)], 7000 + salt + 100 * content + 10 * f
        out.append(_plane(kind, w, h, seed) if ch == 1 else np.stack([_plane(kind, w, h, seed + k) for k in range(3)], -1))
    return np.stack(out)


def expected_maps(oracle, frames, mode, per_channel=False, low=None, high=None):
    """The oracle's maps of a batch: one per frame, three (B, G, R planes, each as a one-channel frame) in per-channel mode."""
    if mode == api.MODE_O:
        lo, hi = (50, 150) if low is None else (low, high)
        return np.stack([oracle.canny_o(f, lo, hi) for f in frames])
    lo, hi = (10, 40) if low is None else (low, high)
    if frames.ndim == 3:
        return oracle.canny_r_batch(frames, lo, hi)
    if per_channel:
        return np.stack([oracle.canny_r(np.ascontiguousarray(f[:, :, k]), lo, hi) for f in frames for k in range(3)])
    return np.stack([oracle.canny_r(f, lo, hi) for f in frames])


# ---- host buffers -------------------------------------------------------------------------------------------------------
def host_view(ptr, nbytes):
    """numpy view of nbytes at ptr.  Of page-locked memory: drop it before the memory is freed, hand on copies only."""
    return np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(ptr))


def split_host_out(raw, n, w, h, row_stride, frame_stride):
    """(maps (n, h, w), every other byte of the buffer) of a copy of hostOut"""
    idx = (np.arange(n) * frame_stride)[:, None, None] + (np.arange(h) * row_stride)[None, :, None] + np.arange(w)[None, None, :]
    mine = np.zeros(raw.size, bool)
    mine[idx.reshape(-1)] = True
    return raw[idx], raw[~mine]


def check_batch(raw, want, w, h, row_stride, frame_stride, what):
    """Every byte of the n = len(want) maps equals the oracle's; every other byte of hostOut -- row padding, gaps, the frames
    beyond n -- is still poison."""
    got, rest = split_host_out(raw, len(want), w, h, row_stride, frame_stride)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        f, y, x = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {want.size} bytes differ; first at map {f} row {y} column {x}: got {int(got[f, y, x])}"
                             f" (0x4D is poison), oracle {int(want[f, y, x])}")
    spoiled = np.flatnonzero(rest != POISON)
    assert spoiled.size == 0, f"{what}: {spoiled.size} bytes of hostOut outside the {len(want)} maps were written"


class Slot:
    def __init__(self, ctx, hin, hout, pinned_in):
        self.ctx, self.hin, self.hout, self.pinned_in = ctx, hin, hout, pinned_in
        self.batch = None   # (index, maps asked for) while a download is in flight


class Ring:
    """with Ring(...) as ring: done = ring.commit(frames) ... done += ring.flush(); every item is (batch index, number of
    maps, copy of the whole hostOut).  pad: extra bytes per host row (both directions), gap: extra bytes between host frames;
    pageable: hc_upload reads a plain numpy array instead of page-locked memory; copy_streams None: left to the caller
    (set_option on every context)."""

    def __init__(self, w, h, ch=1, max_batch=4, depth=3, mode=api.MODE_R, copy_streams=1, pipeline=0, per_channel=0, pad=0, gap=0,
                 pageable=False, thresholds=None):
        self.lib = api.load_library()
        self.w, self.h, self.ch, self.max_batch, self.depth = w, h, ch, max_batch, depth
        self.maps = 3 if per_channel else 1
        self.in_row, self.out_row = w * ch + pad, w + pad
        self.in_fs, self.out_fs = self.in_row * h + gap, self.out_row * h + gap
        self.in_bytes, self.out_bytes = self.in_fs * max_batch, self.out_fs * max_batch * self.maps
        self.order = RingOrder(depth)
        self.slots = []
        try:
            for _ in range(depth):
                ctx = api.Context(w, h, ch, max_batch, mode)
                self.slots.append(Slot(ctx, None, None, not pageable))
                s = self.slots[-1]
                s.hout = self.lib.hc_host_alloc(self.out_bytes)
                s.hin = self.lib.hc_host_alloc(self.in_bytes) if not pageable else np.full(self.in_bytes, POISON, np.uint8)
                assert s.hout and s.hin is not None, api.last_error()
                if per_channel:
                    ctx.set_option(api.OPT_PER_CHANNEL, 1)
                if pipeline:
                    ctx.set_option(api.OPT_PIPELINE, 1)
                if copy_streams is not None:
                    ctx.set_option(api.OPT_COPY_STREAMS, copy_streams)
                if thresholds:
                    ctx.set_thresholds(*thresholds)
        except BaseException:
            self.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def close(self):
        try:
            for s in self.slots:
                if s.batch is not None:   # a download in flight writes into hostOut: it ends before the buffer goes
                    self.lib.hc_download_end(s.ctx.handle)
                    s.batch = None
        finally:
            for s in self.slots:
                s.ctx.close()   # (hc_destroy synchronises the device)
                if s.hout:
                    self.lib.hc_host_free(C.c_void_p(s.hout))
                if s.pinned_in and s.hin:
                    self.lib.hc_host_free(C.c_void_p(s.hin))
                s.hin = s.hout = None
            self.slots = []

    def set_option(self, option, value):
        for s in self.slots:
            s.ctx.set_option(option, value)

    def _stage(self, s, frames):
        n = frames.shape[0]
        dst = host_view(s.hin, self.in_bytes) if s.pinned_in else s.hin
        dst[:] = POISON
        rows = frames.reshape(n, self.h, self.w * self.ch)
        for f in range(n):
            block = dst[f * self.in_fs: f * self.in_fs + self.in_row * self.h].reshape(self.h, self.in_row)
            block[:, :self.w * self.ch] = rows[f]
        return s.hin if s.pinned_in else s.hin.ctypes.data

    # the four calls of a batch one by one (the ordering tests put other work between them) ...
    def upload(self, s, frames):
        src = self._stage(s, frames)
        api._ck(self.lib.hc_upload(s.ctx.handle, C.c_void_p(src), self.in_row, self.in_fs, frames.shape[0]))

    def run(self, s, n):
        s.ctx.run(api.CannyStage.HYSTER, n)

    def begin(self, s, n, index=None):
        """hostOut poisoned, then hc_download_begin of the n frames' maps"""
        host_view(s.hout, self.out_bytes)[:] = POISON
        api._ck(self.lib.hc_download_begin(s.ctx.handle, C.c_void_p(s.hout), self.out_row, self.out_fs, n * self.maps))
        s.batch = (index, n * self.maps)

    def complete(self, s):
        """hc_download_end; (batch index, maps, copy of hostOut)"""
        index, nmaps = s.batch
        s.batch = None
        api._ck(self.lib.hc_download_end(s.ctx.handle))
        return index, nmaps, host_view(s.hout, self.out_bytes).copy()

    # ... and together
    def queue(self, s, frames, index=None):
        """hc_upload, hc_run, hc_download_begin on one slot; returns at once"""
        self.upload(s, frames)
        self.run(s, frames.shape[0])
        self.begin(s, frames.shape[0], index)

    def commit(self, frames):
        i, k, done = self.order.commit()
        s = self.slots[k]
        assert s.batch is None, "the ring reuses a slot whose download is in flight"
        self.queue(s, frames, i)
        return [self.complete(self.slots[done % self.depth])] if done is not None else []

    def flush(self):
        return [self.complete(self.slots[i % self.depth]) for i in self.order.flush()]

    def check(self, item, want, what):
        index, nmaps, raw = item
        assert nmaps == len(want), (what, index, nmaps, len(want))
        check_batch(raw, want, self.w, self.h, self.out_row, self.out_fs, f"{what}, batch {index}")


def stream(ring, batches, frames_of):
    """Every batch of a schedule through the ring; the completed items in completion order."""
    done = []
    for content, n in batches:
        done += ring.commit(frames_of(content)[:n])
    return done + ring.flush()


# ---- the blocker of the ordering tests -------------------------------------------------------------------------------------
# BLOCKER_MATMULS products of two 4096 x 4096 float32 matrices on the caller's stream (the chain of
# test_callers_stream_is_honoured in tests/test_gpu_histogram.py, lengthened from 4).  Measured on an MI355X: the chain of
# 48 runs for 44 ms (32: 29.4 ms); the host queues the calls of a test behind it in 0.06 - 0.14 ms, 0.3 ms where they include
# poisoning a 16.6 MB hostOut, 0.53 ms where they include an hc_set_stream onto a torch stream used for the first time
# (upload, switch, run, download_begin) -- a margin of 80 x at the least, where 10 x is asked for to absorb a busy shared
# host.  Every ordering test prints both figures (pytest -s).
BLOCKER_MATMULS = 48


class Blocker:
    """start(stream): the chain of matmuls on `stream`, and a torch event recorded behind it."""

    def __init__(self):
        import torch
        self.torch = torch
        self.big = torch.ones((4096, 4096), dtype=torch.float32, device="cuda") * 1e-2
        self.out = torch.empty_like(self.big)
        torch.mm(self.big, self.big, out=self.out)   # the first product loads the BLAS kernels: not part of any blocker
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        done = self.start(s)
        b.record(s)
        done.synchronize()
        b.synchronize()
        self.ms = a.elapsed_time(b)
        print(f"[host-fed] blocker: {BLOCKER_MATMULS} matmuls run for {self.ms:.2f} ms")

    def start(self, stream):
        torch = self.torch
        with torch.cuda.stream(stream):
            for _ in range(BLOCKER_MATMULS):
                torch.mm(self.big, self.big, out=self.out)
        ev = torch.cuda.Event()
        ev.record(stream)
        return ev


def still_blocked(ev, t0, blocker, what):
    """The precondition of every ordering test, asserted before its first blocking call: everything has been queued and the
    blocker has not finished.  Otherwise the test has shown nothing, and fails."""
    queued_ms = (time.perf_counter() - t0) * 1e3
    busy = ev.query() is False
    print(f"[host-fed] {what}: calls queued in {queued_ms:.3f} ms, blocker of {blocker.ms:.2f} ms still running: {busy}")
    assert busy, f"blocker too short: it had finished when the calls of {what} were queued ({queued_ms:.3f} ms; it runs for {blocker.ms:.2f} ms)"


def check_new(ring, item, want_new, want_old, what):
    maps = split_host_out(item[2], len(want_new), ring.w, ring.h, ring.out_row, ring.out_fs)[0]
    ring.check(item, want_new, what + (": hostOut holds the maps of the PREVIOUS batch" if np.array_equal(maps, want_old) else ""))


def warm(ring, s, frames, rounds):
    """Completed rounds on the context's own stream: every stream, event and pipeline slot the later calls need exists (a slot
    allocated inside a run synchronises the context stream), and the context holds `frames` and their maps."""
    for _ in range(rounds):
        ring.queue(s, frames)
        ring.complete(s)
    s.ctx.sync()


def download_end_main():
    """ev_down, in a process of its own (tests/test_gpu_host_fed.py starts it with 16 hardware queues, so that no two of its
    streams share one).  X, on a stream the blocker holds busy, has a finished run and calls hc_download_begin: the shared
    D2H stream stalls behind the blocker.  Y, with nothing pending, uploads, runs and calls hc_download_begin; its copy sits
    behind X's.  hc_download_end(Y) returns with Y's maps in hostOut and no poison left; then X's are right too.
    Then the same with Y's run synchronised before the blocker starts: Y's stream is idle while its copy waits behind X's.
    X is a context of 8 frames of 1920 x 1080, so that its 16.6 MB copy (a third of a millisecond) lies ahead of Y's.
    Prints "download end ok" or raises ("blocker too short" when the blocker had finished before everything was queued)."""
    api.load_library()   # (the one HIP runtime of the process, before the oracle and torch ask for it)
    from oracle import oracle as O
    O.build()
    import torch
    w, h, nb = 320, 200, 4
    old = np.stack([synth.natural(w, h, 900 + f) for f in range(nb)])
    new = np.stack([synth.noise(w, h, 950 + f) for f in range(nb)])
    want_old, want_new = O.canny_r_batch(old, 10, 40), O.canny_r_batch(new, 10, 40)
    for f in range(nb):
        assert not np.array_equal(want_old[f], want_new[f])
    xw, xh, xn = 1920, 1080, 8
    xframe = synth.natural(xw, xh, 77)
    xframes, xwant = np.stack([xframe] * xn), np.stack([O.canny_r(xframe, 10, 40)] * xn)
    print(f"[host-fed] GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')}, library {api.LIB_PATH}")
    blocker = Blocker()
    assert blocker.ms < 500.0, f"the blocker runs for {blocker.ms:.1f} ms: every blocker finishes well inside a second"
    s = torch.cuda.Stream()
    with Ring(xw, xh, 1, xn, 1, copy_streams=1) as xring, Ring(w, h, 1, nb, 1, copy_streams=1) as ring:
        x, y = xring.slots[0], ring.slots[0]
        warm(xring, x, xframes, 1)   # X: a finished run
        warm(ring, y, old, 1)
        x.ctx.set_stream(s.cuda_stream)
        ev = blocker.start(s)
        t0 = time.perf_counter()
        xring.begin(x, xn)           # ev_ready2 behind the blocker: g_d2h stalls
        ring.queue(y, new)
        still_blocked(ev, t0, blocker, "X download_begin, Y upload + run + download_begin")
        item = ring.complete(y)
        print(f"[host-fed] hc_download_end(Y) returned after {(time.perf_counter() - t0) * 1e3:.2f} ms, blocker finished: {ev.query()}")
        check_new(ring, item, want_new, want_old, "Y behind X's stalled download")
        xring.check(xring.complete(x), xwant, "X's own download")
        # Once more with Y's run finished before the blocker starts.  Above, Y's kernels share the device with the matmuls and
        # may end only with them, a third of a millisecond ahead of Y's copy: a wait for Y's stream alone would often do.
        # Here Y's stream is idle throughout, so such a wait returns at once, 44 ms before the maps arrive.
        ring.upload(y, old)
        ring.run(y, nb)
        y.ctx.sync()
        ev = blocker.start(s)
        t0 = time.perf_counter()
        xring.begin(x, xn)
        ring.begin(y, nb)
        still_blocked(ev, t0, blocker, "X download_begin, Y download_begin with Y's stream idle")
        item = ring.complete(y)
        print(f"[host-fed] hc_download_end(Y) returned after {(time.perf_counter() - t0) * 1e3:.2f} ms, blocker finished: {ev.query()}")
        check_new(ring, item, want_old, want_new, "Y, idle, behind X's stalled download")
        xring.check(xring.complete(x), xwant, "X's own download, second round")
        x.ctx.use_own_stream()
    print("download end ok")


# ---- two host threads, in a process of their own: the first use of the shared copy streams ---------------------------------
def two_threads_main():
    """Two threads, a ring of 2 contexts each; both ask for HC_OPT_COPY_STREAMS right behind a barrier, in a process in which
    nobody has asked before -- g_h2d / g_d2h are created then, under their mutex.  Each thread streams 6 batches of its own
    content; every map equals the oracle, no call fails, and the error text of one thread survives the other's successes.
    Prints "two threads ok" or raises."""
    import threading
    from oracle import oracle as O
    O.build()
    w, h, nb, nbatches = 320, 200, 4, 6
    barrier = threading.Barrier(2)
    failures, results = [], {}

    def body(t):
        try:
            lib = api.load_library()
            sched = schedule(nbatches, 2, nb, 50 + t)
            frames = {c: content_frames(c, w, h, 1, nb, salt=1000 * (t + 1)) for c in range(NCONTENTS)}
            with Ring(w, h, 1, nb, depth=2, copy_streams=None) as ring:
                barrier.wait(timeout=30)
                ring.set_option(api.OPT_COPY_STREAMS, 1)
                mine = "hc_upload: nframes out of range"
                if t == 0:   # an error of this thread's own, then the other thread's successful calls
                    assert lib.hc_upload(ring.slots[0].ctx.handle, C.c_void_p(ring.slots[0].hin), w, w * h, nb + 1) == -1
                barrier.wait(timeout=30)
                done = stream(ring, sched["batches"], lambda c: frames[c])
                barrier.wait(timeout=30)
                if t == 0:
                    assert lib.hc_last_error().decode() == mine, f"thread 0 reads {lib.hc_last_error().decode()!r}"
                assert [d[0] for d in done] == sched["completes"]
                results[t] = (ring.out_row, ring.out_fs, sched, frames, done)
        except BaseException as e:   # noqa: BLE001  (reported by the main thread)
            failures.append(f"thread {t}: {type(e).__name__}: {e}")
            barrier.abort()

    threads = [threading.Thread(target=body, args=(t,), daemon=True) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=60)   # (two of these stay inside the limit the test gives this process)
        assert not th.is_alive(), "a thread has not joined"
    assert not failures, failures
    for t, (row, fs, sched, frames, done) in results.items():
        for index, nmaps, raw in done:
            c, n = sched["batches"][index]
            check_batch(raw, expected_maps(O, frames[c][:n], api.MODE_R), w, h, row, fs, f"thread {t}, batch {index}")
    assert len(results) == 2
    print("two threads ok")


if __name__ == "__main__":
    download_end_main() if sys.argv[1:] == ["download-end"] else two_threads_main()
