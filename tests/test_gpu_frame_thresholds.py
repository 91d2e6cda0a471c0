"""hc_frame_thresholds_device on the MI355X: frame f of a batched Mode O run equals, bit for bit, the oracle with that frame's
pair -- oracle.canny_o at aperture 3 (k_front8o, k_front_o), tests/canny_o_ext_ref.py at aperture 5 and on given gradients
(k_front_o_ext) -- the pair normalised as hc_set_thresholds normalises it (auto_thr_ref.normalised).

Shapes: widths 250 and 497 (just over one strip of the 4-px and of the 8-px kernels, so the item -> frame decoding has two
strips to get wrong), heights 5 and 66, hc_set_tuning rows per work item 1, 7 and the whole frame, batches of 3 and 5.
One-channel rows that hold no whole 8-pixel groups are staged and stay on k_front8o (HC_FORM_FRONT8O, input_staged = 1);
k_front_o runs on 3-channel input and, on the same ragged widths, under HC_OPT_FRONT_SPLIT 0."""
import numpy as np
import pytest

import auto_thr_ref as R
import canny_o_ext_ref as X
from cudacam_amd import api, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FORM_FRONT_O, FORM_FRONT8O, FORM_O_APERTURE5, FORM_O_GRADIENTS = -1, 3, 6, 7
# per frame: a swapped pair, a negative low, a high above 32767 (no strong pixel: an empty map), (0, 0), a pair above every
# magnitude (empty), an ordinary pair
PAIRS = [(150, 50), (-20, 100), (300, 40000), (0, 0), (32000, 32767), (50, 150), (700, 2000)]
# name -> (channels, HC_OPT_FRONT_SPLIT or None, aperture, gradients, form)
FORMS = {
    "front8o": (1, None, 3, False, FORM_FRONT8O),
    "front_o_bgr": (3, None, 3, False, FORM_FRONT_O),
    "front_o_split0": (1, 0, 3, False, FORM_FRONT_O),
    "aperture5": (1, None, 5, False, FORM_O_APERTURE5),
    "aperture5_bgr": (3, None, 5, False, FORM_O_APERTURE5),
    "gradients": (1, None, 3, True, FORM_O_GRADIENTS),
}
_frames_cache, _want_cache = {}, {}


def _frames(w, h, ch, n):
    key = (w, h, ch, n)
    if key not in _frames_cache:
        def one(k):
            return (synth.natural(w, h, 11 + k), synth.noise(w, h, 12 + k), synth.steps(w, h, 200, "diagonal"), synth.natural(w, h, 14 + k)[::-1].copy(),
                    synth.noise(w, h, 15 + k) // 3)[k % 5]
        fr = [one(k) if ch == 1 else np.stack([one(k), one(k + 1), one(k + 2)], -1) for k in range(n)]
        _frames_cache[key] = np.stack(fr)
        _frames_cache[key].setflags(write=False)
    return _frames_cache[key]


def _oracle(form, frame, pair, l2, premap=False):
    ch, _, aperture, grads, _ = FORMS[form]
    lo, hi = R.normalised(*pair)
    if grads:
        dx, dy = X.sobel_o(frame, 3)
        return X.canny_o_from_gradients(dx, dy, lo, hi, l2, premap)
    if aperture == 5:
        return X.canny_o(frame, lo, hi, ksize=5, l2=l2, premap=premap)
    if premap:
        return O.canny_o_stages(frame, lo, hi, l2)
    return O.canny_o(frame, lo, hi, l2)


def _want(form, w, h, n, l2, shift=0):
    """The reference maps of the batch, frame f with PAIRS[(f + shift) % len(PAIRS)]; computed once per case, shared."""
    key = (form, w, h, n, l2, shift)
    if key not in _want_cache:
        frames = _frames(w, h, FORMS[form][0], n)
        _want_cache[key] = np.stack([_oracle(form, frames[f], PAIRS[(f + shift) % len(PAIRS)], l2) for f in range(n)])
        _want_cache[key].setflags(write=False)
    return _want_cache[key]


def _pairs(n, shift=0):
    return [PAIRS[(f + shift) % len(PAIRS)] for f in range(n)]


def _ctx(form, w, h, n, l2, **kw):
    ch, split, aperture, _, _ = FORMS[form]
    ctx = api.Context(w, h, ch, n, api.MODE_O, front_split=split, **kw)
    if aperture != 3:
        ctx.set_option(api.OPT_APERTURE, aperture)
    if l2:
        ctx.set_option(api.OPT_L2_GRADIENT, 1)
    return ctx


class _Batch:
    """The device side of one batch: frames (or their int16 gradients) at a pitch, output buffers, a threshold table."""

    def __init__(self, form, frames, pad=0, nout=1):
        import torch
        self.form, self.grads = form, FORMS[form][3]
        n, h, w = frames.shape[:3]
        ch = FORMS[form][0]
        self.n, self.h, self.w = n, h, w
        if self.grads:
            gx, gy = zip(*(X.sobel_o(f, 3) for f in frames))
            self.pitch = 2 * w
            self.src = [torch.from_numpy(np.stack(g).astype(np.int16)).cuda() for g in (gx, gy)]
        else:
            self.pitch = w * ch + pad
            buf = np.full((n, h, self.pitch), 0xA5, np.uint8)
            buf[:, :, :w * ch] = frames.reshape(n, h, w * ch)
            self.src = [torch.from_numpy(buf).cuda()]
        self.out = [torch.full((n, h, w), 77, dtype=torch.uint8, device="cuda") for _ in range(nout)]
        self.thr = [None] * nout
        torch.cuda.synchronize()

    def table(self, ctx, pairs, slot=0):
        import torch
        self.thr[slot] = torch.tensor(pairs, dtype=torch.int32, device="cuda").contiguous()
        torch.cuda.synchronize()
        ctx.frame_thresholds_device(self.thr[slot].data_ptr(), len(pairs))

    def run(self, ctx, slot=0, n=None):
        n = self.n if n is None else n
        o = self.out[slot]
        if self.grads:
            ctx.run_gradients_device(self.src[0].data_ptr(), self.src[1].data_ptr(), self.pitch, self.pitch * self.h, o.data_ptr(), self.w, self.w * self.h, n)
        else:
            ctx.run_device(self.src[0].data_ptr(), self.pitch, self.pitch * self.h, o.data_ptr(), self.w, self.w * self.h, n)

    def result(self, ctx, slot=0):
        ctx.sync()
        return self.out[slot].cpu().numpy()


def _diff(got, want, what):
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    per_frame = np.bincount(bad[:, 0], minlength=got.shape[0]).tolist()
    raise AssertionError(f"{what}: {len(bad)} pixels differ, per frame {per_frame}; first {[tuple(int(v) for v in p) for p in bad[:6]]}")


@pytest.mark.parametrize("l2", [False, True], ids=["L1", "L2"])
@pytest.mark.parametrize("form", list(FORMS))
def test_frames_are_cut_with_their_own_pair(form, l2):
    for w, h, n in ((250, 5, 3), (250, 66, 5), (497, 5, 5), (497, 66, 3)):
        frames = _frames(w, h, FORMS[form][0], n)
        want = _want(form, w, h, n, l2)
        assert not want[2].any() and (n == 3 or not want[4].any())   # (300, 40000) and (32000, 32767): empty maps
        with _ctx(form, w, h, n, l2) as ctx:
            b = _Batch(form, frames)
            b.table(ctx, _pairs(n))
            for chunk in (1, 7, 16384):   # rows per work item: 1, 7, the whole frame
                ctx.set_tuning(chunk, 0)
                b.out[0].fill_(77)
                b.run(ctx)
                _diff(b.result(ctx), want, f"{form} {w}x{h} n={n} l2={l2} chunk={chunk}")
                staged, _, ran = ctx.last_run_info()
                assert ran == FORMS[form][4], (form, ran)
                if form == "front8o":
                    assert staged   # tight rows of 250 / 497 pixels hold no whole 8-pixel groups: staged, still k_front8o
            assert ctx.get_thresholds() == (50, 150)   # the context's pair is what it was


def test_pairs_above_every_magnitude_and_high_beyond_the_clamp_give_empty_maps():
    want = _want("front8o", 250, 66, 5, False)
    assert not want[2].any() and not want[4].any() and want[0].any() and want[3].any()


@pytest.mark.parametrize("form", list(FORMS))
def test_pipelined_runs_with_rotated_outputs_and_tables(form):
    """Four consecutive pipelined runs, each into its own output with its own table; width 504: k_front8o writes the
    provisional map (W % 8 == 0), the final maps are exact."""
    w, h, n = 504, 66, 5
    frames = _frames(w, h, FORMS[form][0], n)
    for l2 in (False, True):
        with _ctx(form, w, h, n, l2) as ctx:
            ctx.set_option(api.OPT_PIPELINE, 1)
            b = _Batch(form, frames, nout=4)
            for k in range(4):
                b.table(ctx, _pairs(n, shift=k), slot=k)
                b.run(ctx, slot=k)
                assert ctx.last_run_info()[2] == FORMS[form][4]
            ctx.sync()
            for k in range(4):
                _diff(b.out[k].cpu().numpy(), _want(form, w, h, n, l2, shift=k), f"pipelined {form} l2={l2} run {k}")


@pytest.mark.parametrize("form", ["front8o", "front_o_bgr", "aperture5"])
def test_staged_input_view(form):
    w, h, n = 250, 66, 3
    frames = _frames(w, h, FORMS[form][0], n)
    with _ctx(form, w, h, n, False) as ctx:
        b = _Batch(form, frames, pad=3)   # a pitch that is no multiple of 4
        b.table(ctx, _pairs(n))
        b.run(ctx)
        _diff(b.result(ctx), _want(form, w, h, n, False), f"staged {form}")
        assert ctx.last_run_info()[0] and ctx.last_run_info()[2] == FORMS[form][4]


@pytest.mark.parametrize("l2", [False, True], ids=["L1", "L2"])
@pytest.mark.parametrize("form", list(FORMS))
def test_thresh_tap_is_each_frames_own_tristate_map(form, l2):
    w, h, n = 250, 66, 5
    frames = _frames(w, h, FORMS[form][0], n)
    with _ctx(form, w, h, n, l2) as ctx:
        ctx.set_option(api.OPT_DEBUG_TAPS, 1)
        b = _Batch(form, frames)
        b.table(ctx, _pairs(n))
        b.run(ctx)
        got = b.result(ctx)
        tap = ctx.debug_tap(api.TAP_THRESH, n)
    for f in range(n):
        edges, pre = _oracle(form, frames[f], PAIRS[f], l2, premap=True)
        _diff(tap[f][None], pre[None], f"THRESH tap {form} frame {f}")
        _diff(got[f][None], edges[None], f"edges {form} frame {f}")


def test_null_restores_the_context_pair_and_canny_device_ignores_the_table():
    import torch
    w, h, n = 250, 66, 5
    frames = _frames(w, h, 1, n)
    with _ctx("front8o", w, h, n, False) as ctx:
        ctx.set_thresholds(80, 240)
        b = _Batch("front8o", frames)
        b.run(ctx)
        before = b.result(ctx).copy()
        _diff(before, np.stack([O.canny_o(f, 80, 240) for f in frames]), "context pair")
        b.table(ctx, _pairs(n))
        b.run(ctx)
        with_table = b.result(ctx).copy()
        _diff(with_table, _want("front8o", w, h, n, False), "table")
        # hc_canny_device between two table runs: its own thresholds, the table stays in force
        out = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.canny_device(b.src[0].data_ptr(), b.pitch, b.pitch * h, out.data_ptr(), w, w * h, n, 10, 20)
        ctx.sync()
        _diff(out.cpu().numpy(), np.stack([O.canny_o(f, 10, 20) for f in frames]), "canny_device with a table installed")
        b.out[0].fill_(77)
        b.run(ctx)
        _diff(b.result(ctx), with_table, "table run after canny_device")
        assert ctx.get_thresholds() == (80, 240)
        ctx.frame_thresholds_device(None)
        b.out[0].fill_(77)
        b.run(ctx)
        assert np.array_equal(b.result(ctx), before), "NULL does not restore the context's pair"


def test_hc_run_on_uploaded_frames_reads_the_table():
    import torch
    w, h, n = 497, 66, 3
    frames = _frames(w, h, 1, n)
    thr = torch.tensor(_pairs(n), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with _ctx("front8o", w, h, n, False) as ctx:
        ctx.frame_thresholds_device(thr.data_ptr(), n)
        _diff(ctx.process(frames), _want("front8o", w, h, n, False), "hc_run with a table")


def test_argument_errors():
    import torch
    thr = torch.zeros((8, 2), dtype=torch.int32, device="cuda")
    with api.Context(64, 48, 1, 4, api.MODE_R) as ctx:
        with pytest.raises(api.HipCannyError, match="error -1"):
            ctx.frame_thresholds_device(thr.data_ptr(), 2)   # a mode R context
    with api.Context(64, 48, 1, 4, api.MODE_O) as ctx:
        for ptr, n in ((thr.data_ptr() + 2, 2), (thr.data_ptr() + 1, 2), (thr.data_ptr(), 0), (thr.data_ptr(), -1), (thr.data_ptr(), 5)):
            with pytest.raises(api.HipCannyError, match="error -1"):
                ctx.frame_thresholds_device(ptr, n)
        ctx.frame_thresholds_device(thr.data_ptr(), 2)
        frames = _frames(64, 48, 1, 3)
        with pytest.raises(api.HipCannyError, match="error -1"):   # a run longer than the table
            ctx.process(frames)
        d = torch.from_numpy(frames.copy()).cuda()
        out = torch.zeros((3, 48, 64), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(api.HipCannyError, match="error -1"):
            ctx.run_device(d.data_ptr(), 64, 64 * 48, out.data_ptr(), 64, 64 * 48, 3)
        ctx.run_device(d.data_ptr(), 64, 64 * 48, out.data_ptr(), 64, 64 * 48, 2)   # two frames fit
        ctx.sync()
        ctx.frame_thresholds_device(None)
        ctx.run_device(d.data_ptr(), 64, 64 * 48, out.data_ptr(), 64, 64 * 48, 3)
        ctx.sync()
        _diff(out.cpu().numpy(), np.stack([O.canny_o(f, 50, 150) for f in frames]), "after NULL")
