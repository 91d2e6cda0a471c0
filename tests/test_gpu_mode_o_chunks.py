"""The 4-px Mode O front kernels at every work-item length: k_front_o (form -1: 3-channel input, or HC_OPT_FRONT_SPLIT 0) and
k_front_o_ext (form 6: aperture 5; form 7: caller-given dx / dy).  All three cut a frame into work items of chunk_rows
rows; each item restarts its register rings, repeats a warm-up, prefetches six rows ahead with the row index clamped to
the last row it needs, and loops in trips of six steps that overshoot its end.  The automatic split keeps small batches at
16 rows or fewer per item, so this file sets the length itself (hc_set_tuning: 1 .. more than the frame) and runs the
batch sizes at which the automatic rule gives one and two items per strip (pinned in tests/cpp/plan_driver.cpp).

Bit for bit, before the flood (HC_TAP_THRESH: the bit planes these kernels write themselves) and after it, against the
oracle (aperture 3) and tests/canny_o_ext_ref.py (aperture 5, gradients).  Every frame used has, in the reference, a
candidate and an empty pixel in every row, so every seam of every length has something to get wrong."""
import numpy as np
import pytest

from cudacam_amd import api, synth
import canny_o_ext_ref as X
from test_gpu_canny_o_ext import _diff, _rand_grad

pytestmark = pytest.mark.gpu

H_SEAMS = 41
SHAPES = [(500, H_SEAMS), (249, H_SEAMS), (5, 7)]   # three strips, the last ragged, W % 4 == 0 / a second strip of one column / tiny
# for H = 41: every residue mod 6 (the ring period), a last item of one row (8, 20, 40), lengths above 16, the frame, beyond it
CHUNKS = [1, 2, 3, 4, 5, 6, 7, 8, 11, 12, 13, 17, 20, 21, 40, 41, 42, 100]
# seeds for which, in the reference, every row of every frame is mixed (asserted on the CPU before anything runs); rows of
# five pixels need a seed per form: {(form, channels, L2): seed}
SEEDS = {(500, 41): 1, (249, 41): 1, (64, 26): 1,
         (5, 7): {(-1, 1, False): 12, (-1, 1, True): 12, (-1, 3, False): 10, (-1, 3, True): 6, (6, 1, False): 12, (6, 1, True): 7,
                  (6, 3, False): 1, (6, 3, True): 1, (7, 1, False): 49, (7, 1, True): 49, (7, 3, False): 48, (7, 3, True): 25}}
THR3, THR5, THR_FULL = (30, 90), (250, 750), (20000, 30000)   # Sobel 3 / Sobel 5 / full-range int16 gradients

FORMS = [("front_o-mono", -1, 1), ("front_o-bgr", -1, 3), ("aperture5-mono", 6, 1), ("aperture5-bgr", 6, 3),
         ("gradients-mono", 7, 1), ("gradients-bgr", 7, 3)]


def _stripes(w, h, phase=0):
    """Diagonal bands six pixels wide, "/" on the left half and "\\" on the right: both diagonal NMS branches in every row."""
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.where(xx < (w + 1) // 2, xx + yy, xx - yy + 6 * h) + phase
    return (((d // 6) & 1) * 200 + 20).astype(np.uint8)


def _mono_frames(w, h, seed):
    """Four different frames: natural, noise, diagonal stripes, noise."""
    return [synth.natural(w, h, seed), synth.noise(w, h, seed + 1), _stripes(w, h, seed), synth.noise(w, h, seed + 2)]


def _u8_frames(w, h, ch, seed):
    m = _mono_frames(w, h, seed)
    if ch == 1:
        return m
    return [np.stack([m[k], m[(k + 1) % 4], m[(k + 2) % 4][::-1]], -1) for k in range(4)]


class Batch:
    """What one run gets (u8 frames, or int16 dx / dy), its thresholds, and what the reference makes of it."""

    def __init__(self, oracle, form, l2, low, high, frames=None, grads=None):
        self.low, self.high = low, high
        if form == 7:
            self.dx = np.stack([np.asarray(a, np.int16) for a, _ in grads])
            self.dy = np.stack([np.asarray(b, np.int16) for _, b in grads])
            assert all(np.array_equal(self.dx[k], a) and np.array_equal(self.dy[k], b) for k, (a, b) in enumerate(grads))
            ref = [X.canny_o_from_gradients(a, b, low, high, l2, premap=True) for a, b in grads]
        else:
            self.frames = np.stack(frames)
            if form == 6:
                ref = [X.canny_o(f, low, high, ksize=5, l2=l2, premap=True) for f in frames]
            else:
                ref = [oracle.canny_o_stages(f, low, high, l2) for f in frames]
        self.edges = np.stack([e for e, _ in ref])
        self.pre = np.stack([p for _, p in ref])
        self.n = len(ref)

    def assert_every_row_mixed(self, what):
        """Non-vacuity, on the reference alone: a candidate-or-strong pixel and an empty one in every row of every frame."""
        busy, empty = (self.pre != 0).any(axis=2), (self.pre == 0).any(axis=2)
        assert busy.all() and empty.all(), f"{what}: rows without a candidate {np.argwhere(~busy).tolist()}, without an empty pixel {np.argwhere(~empty).tolist()}"


def _seed(w, h, form, ch, l2):
    s = SEEDS[(w, h)]
    return s[(form, ch, l2)] if isinstance(s, dict) else s


def _batches(oracle, form, ch, l2, w, h):
    """Batches of two frames with different content.  u8 forms: (natural, noise), (stripes, noise); gradients: the Sobel 3
    of the first pair, the Sobel 5 of the second, and two frames of full-range random int16 pairs."""
    seed = _seed(w, h, form, ch, l2)
    f = _u8_frames(w, h, ch, seed)
    if form != 7:
        low, high = THR5 if form == 6 else THR3
        return [Batch(oracle, form, l2, low, high, frames=f[0:2]), Batch(oracle, form, l2, low, high, frames=f[2:4])]
    rx, ry = _rand_grad((2, h, w) if ch == 1 else (2, h, w, 3), seed + 3)
    return [Batch(oracle, 7, l2, *THR3, grads=[X.sobel_o(v, 3) for v in f[0:2]]),
            Batch(oracle, 7, l2, *THR5, grads=[X.sobel_o(v, 5) for v in f[2:4]]),
            Batch(oracle, 7, l2, *THR_FULL, grads=[(rx[0], ry[0]), (rx[1], ry[1])])]


def _ctx(w, h, ch, nb, form, l2, taps):
    ctx = api.Context(w, h, ch, nb, api.MODE_O, front_split=0 if form == -1 and ch == 1 else None)
    if form == 6:
        ctx.set_option(api.OPT_APERTURE, 5)
    ctx.set_option(api.OPT_L2_GRADIENT, int(l2))
    if taps:
        ctx.set_option(api.OPT_DEBUG_TAPS, 1)
    return ctx


def _process(ctx, form, b):
    ctx.set_thresholds(b.low, b.high)
    return ctx.process_gradients(b.dx, b.dy) if form == 7 else ctx.process(b.frames)


def _pipelined(ctx, form, ch, w, h, seq, d_in, d_out, what):
    """Three runs into two outputs used in turn; the last two maps are checked, then refilled with stale bytes."""
    for r, k in enumerate(seq):
        ctx.set_thresholds(d_in[k][0].low, d_in[k][0].high)
        o = d_out[r % 2]
        if form == 7:
            ctx.run_gradients_device(d_in[k][1].data_ptr(), d_in[k][2].data_ptr(), 2 * w * ch, 2 * w * ch * h, o.data_ptr(), w, w * h, 2)
        else:
            ctx.run_device(d_in[k][1].data_ptr(), w * ch, w * ch * h, o.data_ptr(), w, w * h, 2)
    ctx.sync()
    assert ctx.last_run_info()[2] == form
    for r in (1, 2):
        _diff(d_out[r % 2].cpu().numpy(), d_in[seq[r]][0].edges, f"{what} pipelined run {r}")
        d_out[r % 2].fill_(0x5A + r)   # stale bytes must not survive the next pass


@pytest.mark.parametrize("l2", [False, True], ids=["L1", "L2"])
@pytest.mark.parametrize("name,form,ch", FORMS, ids=[f[0] for f in FORMS])
def test_every_chunk_length(oracle, name, form, ch, l2):
    """Every work-item length on small frames, plain (bit planes and edges); the 500-column shape also pipelined, where
    k_front_o writes the provisional map (W % 4 == 0)."""
    import torch
    cases = {(w, h): _batches(oracle, form, ch, l2, w, h) for w, h in SHAPES}
    for (w, h), batches in cases.items():
        for k, b in enumerate(batches):
            b.assert_every_row_mixed(f"{name} {w}x{h} batch {k}")
    for (w, h), batches in cases.items():
        with _ctx(w, h, ch, 2, form, l2, taps=True) as ctx:
            for chunk in CHUNKS:
                ctx.set_tuning(chunk, 0)
                for k, b in enumerate(batches):
                    what = f"{name} L2 {l2} {w}x{h} chunk {chunk} batch {k}"
                    got = _process(ctx, form, b)
                    assert ctx.last_run_info()[2] == form
                    _diff(ctx.debug_tap(api.TAP_THRESH, b.n), b.pre, what + ": bit planes")
                    _diff(got, b.edges, what + ": edges")
    w, h = SHAPES[0]
    batches = cases[(w, h)]
    if form == 7:
        d_in = [(b, torch.from_numpy(b.dx).cuda(), torch.from_numpy(b.dy).cuda()) for b in batches]
    else:
        d_in = [(b, torch.from_numpy(b.frames).cuda()) for b in batches]
    d_out = [torch.full((2, h, w), 0x5A, dtype=torch.uint8, device="cuda") for _ in range(2)]
    seq = [r % len(batches) for r in range(3)]
    torch.cuda.synchronize()
    with _ctx(w, h, ch, 2, form, l2, taps=False) as ctx:
        ctx.set_option(api.OPT_PIPELINE, 1)
        for chunk in CHUNKS:
            ctx.set_tuning(chunk, 0)
            _pipelined(ctx, form, ch, w, h, seq, d_in, d_out, f"{name} L2 {l2} {w}x{h} chunk {chunk}")


BIG_W, BIG_H = 64, 26   # one strip; 12288 frames: one item spans the frame, 6144: two items of 13 rows (plan_driver.cpp pins both)


@pytest.mark.parametrize("l2", [False, True], ids=["L1", "L2"])
@pytest.mark.parametrize("name,form,ch", [FORMS[1], FORMS[2], FORMS[4]], ids=[FORMS[1][0], FORMS[2][0], FORMS[4][0]])
def test_plans_of_big_batches(oracle, name, form, ch, l2):
    """hc_set_tuning untouched: the work split big batches really get -- one or two items per strip, which no small batch
    reaches.  Frames tiled from four distinct ones; frames 0 .. 3 and the last are checked."""
    w, h = BIG_W, BIG_H
    f = _u8_frames(w, h, ch, _seed(w, h, form, ch, l2))   # natural, noise, stripes, noise
    if form == 7:
        ref = Batch(oracle, 7, l2, *THR3, grads=[X.sobel_o(v, 3) for v in f])
        src = (ref.dx, ref.dy)
    else:
        ref = Batch(oracle, form, l2, *(THR5 if form == 6 else THR3), frames=f)
        src = (ref.frames,)
    ref.assert_every_row_mixed(f"{name} {w}x{h}")
    edges, pre = ref.edges, ref.pre
    with _ctx(w, h, ch, 12288, form, l2, taps=True) as ctx:
        ctx.set_thresholds(ref.low, ref.high)
        for n in (12288, 6144):
            tiled = [np.tile(a, (n // 4,) + (1,) * (a.ndim - 1)) for a in src]
            got = ctx.process_gradients(*tiled) if form == 7 else ctx.process(tiled[0])
            assert ctx.last_run_info()[2] == form
            tap = ctx.debug_tap(api.TAP_THRESH, n)
            for k in (0, 1, 2, 3, n - 1):
                _diff(tap[k], pre[k % 4], f"{name} L2 {l2} {n} frames, frame {k}: bit planes")
                _diff(got[k], edges[k % 4], f"{name} L2 {l2} {n} frames, frame {k}: edges")
