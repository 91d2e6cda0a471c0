"""The path a real host takes -- hc_upload, hc_run, hc_download_begin / hc_download_end on several contexts at once, with
HC_OPT_COPY_STREAMS -- checked map by map against the oracle (tests/host_fed_ring.py is the ring).

Parity: rings of 3 contexts that wrap three times and end on a ragged batch, every mode and channel form, copy streams on and
off, plain and pipelined, tight and pitched internal rows, padded host rows, a pageable upload source.

Ordering: each wait of the event graph between the context streams and the two shared copy streams (ev_ready, ev_up,
ev_ready2 / ev_done, ev_down, the repeated copy after a host-side continuation, a switch of the context stream behind an
upload) has a test that FORCES the order it guards against: a chain of large torch matmuls (the blocker) holds a caller's
stream busy while every asynchronous call of the test is queued, and the test asserts that the blocker was still running
when the last of them had returned ("blocker too short" otherwise: a failure, never a pass).  Without its wait the library
returns the previous batch's maps, or poison, every time."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import host_fed_ring as HR
from cudacam_amd import api, synth

pytestmark = pytest.mark.gpu

H, NB, DEPTH, NBATCHES = 200, 4, 3, 11   # the ring wraps three times (11 batches on 3 slots) and ends on a ragged batch
SCHED = HR.schedule(NBATCHES, DEPTH, NB, 2026)
# name: (mode, channels, HC_OPT_PER_CHANNEL)
FORMS = {"R-1ch": (api.MODE_R, 1, 0), "R-bgr": (api.MODE_R, 3, 0), "R-bgr-per-channel": (api.MODE_R, 3, 1), "O-1ch": (api.MODE_O, 1, 0),
         "O-bgr": (api.MODE_O, 3, 0)}
HC_E_STATE = -3

# ---- references, computed once --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refs(oracle):
    """(form, width) -> ({content: frames}, {content: oracle maps}) of NB frames per content; never modified"""
    cache = {}

    def get(form, w):
        if (form, w) not in cache:
            mode, ch, pc = FORMS[form]
            frames = {c: HR.content_frames(c, w, H, ch, NB) for c in range(HR.NCONTENTS)}
            want = {c: HR.expected_maps(oracle, frames[c], mode, bool(pc)) for c in frames}
            for a in list(frames.values()) + list(want.values()):
                a.setflags(write=False)
            cache[(form, w)] = (frames, want)
        return cache[(form, w)]
    return get


def _stream_and_check(ring, refs, form, w, what, batches=SCHED["batches"], completes=None):
    frames, want = refs(form, w)
    done = HR.stream(ring, batches, lambda c: frames[c])
    assert [d[0] for d in done] == (list(range(len(batches))) if completes is None else completes), "batches came back out of order"
    for item in done:
        c, n = batches[item[0]]
        ring.check(item, want[c][:n * ring.maps], what)


# ---- 2. ring parity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", [0, 1])
@pytest.mark.parametrize("copy_streams", [1, 0])
@pytest.mark.parametrize("w", [320, 324])   # internal rows tight (a batch is one 1-D DMA) / pitched to 256 (2-D copies, frame by frame)
@pytest.mark.parametrize("form", list(FORMS))
def test_ring_parity(refs, form, w, copy_streams, pipeline):
    mode, ch, pc = FORMS[form]
    with HR.Ring(w, H, ch, NB, DEPTH, mode, copy_streams, pipeline, pc) as ring:
        _stream_and_check(ring, refs, form, w, f"{form} {w}x{H} copy_streams={copy_streams} pipeline={pipeline}", completes=SCHED["completes"])


@pytest.mark.parametrize("pipeline", [0, 1])
@pytest.mark.parametrize("copy_streams", [1, 0])
@pytest.mark.parametrize("variant", ["padded-rows", "pageable-source"])
def test_ring_parity_host_layouts(refs, variant, copy_streams, pipeline):
    """Host rows of w + 12 bytes with a gap between the frames (the 2-D path, at a width whose internal rows are tight; the
    padding and the gaps of hostOut stay poison), and a plain numpy array as the upload source, as Context.upload passes."""
    kw = dict(pad=12, gap=40) if variant == "padded-rows" else dict(pageable=True)
    with HR.Ring(320, H, 1, NB, DEPTH, api.MODE_R, copy_streams, pipeline, **kw) as ring:
        _stream_and_check(ring, refs, "R-1ch", 320, f"{variant} copy_streams={copy_streams} pipeline={pipeline}")


def test_copy_streams_switched_between_batches(refs):
    """HC_OPT_COPY_STREAMS 1 -> 0 -> 1 between batches of the same contexts: the same maps."""
    with HR.Ring(320, H, 1, NB, DEPTH, copy_streams=1) as ring:
        for k, value in enumerate((1, 0, 1, 0, 1)):
            ring.set_option(api.OPT_COPY_STREAMS, value)
            batches = SCHED["batches"][2 * k: 2 * k + 4]
            ring.order = HR.RingOrder(DEPTH)
            _stream_and_check(ring, refs, "R-1ch", 320, f"phase {k}, copy_streams={value}", batches=batches)


def test_copy_streams_refused_while_a_download_is_in_flight(refs):
    frames, want = refs("R-1ch", 320)
    lib = api.load_library()
    for value in (1, 0):
        with HR.Ring(320, H, 1, NB, 1, copy_streams=value) as ring:
            s = ring.slots[0]
            ring.queue(s, frames[2], 0)
            for other in (0, 1):
                assert lib.hc_set_option(s.ctx.handle, api.OPT_COPY_STREAMS, other) == HC_E_STATE
                assert "a download is in flight" in lib.hc_last_error().decode()
            ring.check(ring.complete(s), want[2], f"refused switch, copy_streams={value}")
            ring.queue(s, frames[3][:3], 1)   # the option is what it was: the next batch takes the same path
            ring.check(ring.complete(s), want[3][:3], f"after the refused switch, copy_streams={value}")
            s.ctx.set_option(api.OPT_COPY_STREAMS, 1 - value)   # nothing in flight: accepted


# ---- 3. ordering ----------------------------------------------------------------------------------------------------------
W = 320


@pytest.fixture(scope="module")
def blocker():
    b = HR.Blocker()   # (the chain, its length and the measured times: host_fed_ring.py)
    assert b.ms < 500.0, f"the blocker runs for {b.ms:.1f} ms: every blocker finishes well inside a second"
    return b


@pytest.fixture(scope="module")
def old_new(oracle):
    """Two batches of NB frames that differ in every frame -- natural frames (old), noise (new) -- and their oracle maps."""
    old = np.stack([synth.natural(W, H, 900 + f) for f in range(NB)])
    new = np.stack([synth.noise(W, H, 950 + f) for f in range(NB)])
    want_old, want_new = oracle.canny_r_batch(old, 10, 40), oracle.canny_r_batch(new, 10, 40)
    for f in range(NB):
        assert not np.array_equal(want_old[f], want_new[f])
    for a in (old, new, want_old, want_new):
        a.setflags(write=False)
    return old, new, want_old, want_new


def _device_ptrs(ctx):
    a, b, ip, op, ifs, ofs = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
    api._ck(ctx.lib.hc_device_ptrs(ctx.handle, C.byref(a), C.byref(b), C.byref(ip), C.byref(op), C.byref(ifs), C.byref(ofs)))
    return a.value, b.value, ip.value, op.value, ifs.value, ofs.value


def _poison_output(ctx, nmaps=NB):
    """The context's internal output buffer filled with poison, and waited for."""
    d_out, ofs = _device_ptrs(ctx)[1], _device_ptrs(ctx)[5]
    ctx.sync()
    hip = api.preload_hip_runtime() or C.CDLL("libamdhip64.so")
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    assert hip.hipMemset(d_out, HR.POISON, ofs * nmaps) == 0
    assert hip.hipDeviceSynchronize() == 0


_still_blocked, _check_new, _warm = HR.still_blocked, HR.check_new, HR.warm


@pytest.mark.parametrize("pipeline", [0, 1])
def test_download_waits_for_the_run(old_new, blocker, pipeline):
    """ev_ready2, and pipelined hc_download_begin's wait of the context stream for the slot's ev_done ahead of it: the copy on
    the shared D2H stream leaves after the run that a busy context stream holds back -- not at once, with the old maps or
    poison.  (queue_download's own wait for ev_done is covered by that one: removing it alone changes nothing, removing
    both fails the pipelined case.)"""
    import torch
    old, new, want_old, want_new = old_new
    s = torch.cuda.Stream()
    with HR.Ring(W, H, 1, NB, 1, copy_streams=1, pipeline=pipeline) as ring:
        x = ring.slots[0]
        _warm(ring, x, old, 5 if pipeline else 1)
        _poison_output(x.ctx)
        x.ctx.set_stream(s.cuda_stream)
        ring.upload(x, new)
        ev = blocker.start(s)
        t0 = time.perf_counter()
        ring.run(x, NB)
        ring.begin(x, NB)
        _still_blocked(ev, t0, blocker, f"run + download_begin (pipeline={pipeline})")
        item = ring.complete(x)
        assert x.ctx.hysteresis_totals()[1] == 0   # (no host-side continuation: its repeated copy would hide a copy that left early)
        _check_new(ring, item, want_new, want_old, f"download behind a blocked run, pipeline={pipeline}")
        x.ctx.use_own_stream()


def test_run_waits_for_its_upload_behind_another_contexts_copy(old_new, blocker):
    """ev_up: X's upload stalls the shared H2D stream behind X's busy stream; Y's upload queues behind it, and Y's run -- on
    Y's own, idle stream -- must wait for it instead of reading the batch Y still holds."""
    import torch
    old, new, want_old, want_new = old_new
    s = torch.cuda.Stream()
    with HR.Ring(W, H, 1, NB, 2, copy_streams=1) as ring:
        x, y = ring.slots
        _warm(ring, x, old, 1)
        _warm(ring, y, old, 1)   # Y holds old in d_in
        _poison_output(y.ctx)
        x.ctx.set_stream(s.cuda_stream)
        ev = blocker.start(s)
        t0 = time.perf_counter()
        ring.upload(x, old)      # hipStreamQuery(s): busy -> behind ev_ready, i.e. behind the blocker, on g_h2d
        ring.upload(y, new)
        ring.run(y, NB)
        ring.begin(y, NB)
        _still_blocked(ev, t0, blocker, "X upload, Y upload + run + download_begin")
        item = ring.complete(y)
        x.ctx.sync()
        _check_new(ring, item, want_new, want_old, "Y behind X's stalled upload")
        x.ctx.use_own_stream()


def test_download_end_waits_for_its_own_copy_on_the_shared_stream():
    """ev_down: X's download stalls the shared D2H stream behind X's busy stream, Y's copy sits behind it;
    hc_download_end(Y) must return only when Y's maps have arrived, not when Y's own stream is idle
    (host_fed_ring.download_end_main).  In a process of its own with 16 hardware queues: streams that share a hardware queue
    are ordered by it, so that with the 4 of HIP's default a synchronisation of Y's stream may cover the copy stream as well
    and hide a missing wait; with 16 every stream of that process (8) has a queue to itself.  Two rounds: Y's run queued
    behind the blocker's start, and Y's run finished before it, so that Y's stream is idle while its copy waits.  Measured
    with hipEventSynchronize(ev_down) replaced by hipStreamSynchronize(context stream), through this test: the second round
    returns after 0.62 ms, the blocker still running, with all 256000 bytes of Y's hostOut poison (the first round is a
    race the mutation can win: Y's kernels end with the matmuls, 0.3 ms ahead of the copy)."""
    out = subprocess.run([sys.executable, HR.__file__, "download-end"], capture_output=True, text=True, timeout=180,
                         env=dict(os.environ, GPU_MAX_HW_QUEUES="16"))
    print(out.stdout[-2000:])
    assert out.returncode == 0 and "download end ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_upload_waits_for_a_reader_of_the_input_on_the_context_stream(old_new, blocker):
    """ev_ready: a histogram of the context's own input buffer is queued on its busy stream; the next upload, on the shared
    H2D stream, must not overwrite the frames under it."""
    import torch
    old, new, want_old, want_new = old_new
    s = torch.cuda.Stream()
    hist = torch.zeros((NB, 256), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with HR.Ring(W, H, 1, NB, 1, copy_streams=1) as ring:
        x = ring.slots[0]
        _warm(ring, x, old, 1)
        d_in, _, in_pitch, _, in_fs, _ = _device_ptrs(x.ctx)
        x.ctx.set_stream(s.cuda_stream)
        ring.upload(x, old)
        x.ctx.histogram_device(d_in, in_pitch, in_fs, NB, hist.data_ptr())   # (the first call of the entry on this context)
        x.ctx.sync()
        hist.fill_(-1)
        torch.cuda.synchronize()
        ev = blocker.start(s)
        t0 = time.perf_counter()
        x.ctx.histogram_device(d_in, in_pitch, in_fs, NB, hist.data_ptr())
        ring.upload(x, new)
        _still_blocked(ev, t0, blocker, "histogram of d_in + upload")
        x.ctx.sync()
        got = hist.cpu().numpy()
        want = np.stack([np.bincount(f.reshape(-1), minlength=256) for f in old])
        if not np.array_equal(got, want):
            f, b = (int(v) for v in np.argwhere(got != want)[0])
            nxt = np.array_equal(got, np.stack([np.bincount(q.reshape(-1), minlength=256) for q in new]))
            raise AssertionError(f"histogram of the batch before the upload: first difference at frame {f} bin {b}: got {int(got[f, b])}, numpy {int(want[f, b])}"
                                 + ("; the histogram counted the NEXT batch: the upload overtook it" if nxt else ""))
        ring.run(x, NB)
        ring.begin(x, NB)
        _check_new(ring, ring.complete(x), want_new, want_old, "the run after the upload")
        x.ctx.use_own_stream()


@pytest.fixture(scope="module")
def continuation_case(oracle):
    """The frames of test_download_end_after_a_continuation_elsewhere (tests/test_gpu_parity.py): with one hysteresis launch
    queued, the first frame needs 18 and is continued from the host."""
    w, h = 1000, 2300
    line = np.zeros((h, w), np.uint8)
    line[:, 100:140] = 20
    for r in range(20):
        line[r, 100:140] = 120 - 5 * r
    frames = np.stack([line, synth.natural(w, h, 79)])
    want = oracle.canny_r_batch(frames, 10, 40, threads=4)
    frames.setflags(write=False)
    want.setflags(write=False)
    return w, h, frames, want


@pytest.mark.parametrize("between", ["sync", "totals", "upload", "download_end"])
def test_stale_copy_is_repeated_on_the_copy_stream(continuation_case, between):
    """A host-side continuation between hc_download_begin and hc_download_end -- in hc_sync, hc_hysteresis_totals, hc_upload,
    or in hc_download_end itself -- rewrites maps whose copy is already on the shared D2H stream: hc_download_end queues the
    copy again there, records ev_down again and waits for THAT."""
    w, h, frames, want = continuation_case
    with HR.Ring(w, h, 1, 2, 1, copy_streams=1) as ring:
        x = ring.slots[0]
        x.ctx.set_tuning(0, 1)   # one launch queued, a frame that needs 18: continued from the host
        x.ctx.hysteresis_totals(reset=True)
        ring.queue(x, frames, 0)
        continued = 0
        if between == "sync":
            x.ctx.sync()
        elif between == "totals":
            continued = x.ctx.hysteresis_totals(reset=True)[1]
        elif between == "upload":   # from the frames themselves: hostIn may still be read by the first upload, and is not restaged
            api._ck(ring.lib.hc_upload(x.ctx.handle, C.c_void_p(frames.ctypes.data), w, w * h, 2))
        item = ring.complete(x)
        continued += x.ctx.hysteresis_totals()[1]
        assert continued == 1, "the one-launch run was not continued from the host"
        ring.check(item, want, f"download_begin, {between}, download_end with copy streams")


@pytest.mark.parametrize("copy_streams", [0, 1])
@pytest.mark.parametrize("switch", ["set_stream", "use_own_stream"])
def test_upload_then_stream_switch_then_run(old_new, blocker, switch, copy_streams):
    """hc_set_stream / hc_use_own_stream order the incoming stream behind the outgoing one: an upload queued on a busy stream
    (directly, or through ev_ready on the shared H2D stream) is seen by the run queued on the other stream after the switch."""
    import torch
    old, new, want_old, want_new = old_new
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with HR.Ring(W, H, 1, NB, 1, copy_streams=copy_streams) as ring:
        x = ring.slots[0]
        _warm(ring, x, old, 1)
        _poison_output(x.ctx)
        x.ctx.set_stream(s1.cuda_stream)
        ev = blocker.start(s1)
        t0 = time.perf_counter()
        ring.upload(x, new)
        if switch == "set_stream":
            x.ctx.set_stream(s2.cuda_stream)
        else:
            x.ctx.use_own_stream()
        ring.run(x, NB)
        ring.begin(x, NB)
        _still_blocked(ev, t0, blocker, f"upload, {switch}, run + download_begin (copy_streams={copy_streams})")
        _check_new(ring, ring.complete(x), want_new, want_old, f"upload, {switch}, run: copy_streams={copy_streams}")
        x.ctx.use_own_stream()


def test_two_host_threads_first_use_of_the_copy_streams():
    """host_fed_ring.two_threads_main in a process of its own: only there are the shared copy streams still to be created
    when the two threads ask for them behind a barrier."""
    out = subprocess.run([sys.executable, HR.__file__], capture_output=True, text=True, timeout=180)   # (the child's own limits add up to less)
    assert out.returncode == 0 and "two threads ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
