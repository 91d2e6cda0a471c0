"""hc_pyr_down_device (k_pyr_down8) and hc_lk_flow_device (k_lk_flow) on the MI355X, bit for bit against tests/flow_ref.py (anchored
by tests/test_flow_ref_cpu.py, which also asserts what each case below is for, on the reference alone; the cases themselves are in
tests/flow_cases.py): planes compared as bytes, points and err as their uint32 words, status exactly.  No tolerances.
  pyr_down   guarded arenas (tests/view_arena.py): every byte around the destination rows is compared with what it held before.
             Sizes at lane, dword, strip and chunk seams: widths 246 .. 254 (the right border within 2 columns of a strip's last
             lanes and of its halo lane), 257, 496, 497; heights 63 .. 66 and 70 (the bottom reflection at a chunk's end and in the
             next chunk's warm-up); 2 x 2 and 3 x 3 strips and chunks with 3 frames; every alignment of both sides; ROIs; an
             all-255 plane in every shape.
  lk_flow    guard words around every array, the images in one arena of random bytes that is compared whole.  All 14 windows, so
             each of the six compiled kernels and every window with idle rounds; points at the borders, at the out-of-frame rule,
             on flat content, NaN and far away; counts below, at and above the capacity; the half-step stop; 64 iterations; levels
             0, 1, 2 and 15 alone; planes of 1 x 1, 1 x 9, 9 x 1 and 6 x 5; pitched and offset views, a frame stride beyond the
             frame, next as the frame behind prev in one ring, both as ROIs of one plane; window sums beyond 32 bits.
  order      both entries behind pipelined runs whose maps are not final until the host has continued them (the apparatus of
             tests/device_op_sequences.py): reading a pending output, writing into one, prev and next in two of them; runs that
             write elsewhere stay in flight; neither entry is a run; stream switches inside a chain; every call twice.
  Python     Context.pyr_down, optical_flow (also where the pyramid must stop early) and track against the chained references.
Not here: thinning, corners and flow in the seeded chains of tests/device_op_sequences.py."""
import numpy as np
import pytest

from cudacam_amd import api, synth
import flow_cases as FC
import flow_ref as R
import view_arena as VA

pytestmark = pytest.mark.gpu

GUARD = 0xA5A5A5A5


# ---- cv::pyrDown ---------------------------------------------------------------------------------------------------------------
def _pyr(ctx, src, pitch=None, fs=None, off=0, out_pitch=None, out_fs=None, out_off=0, seed=0):
    import torch
    n, h, w = src.shape
    dh, dw = (h + 1) // 2, (w + 1) // 2
    pitch = w if pitch is None else pitch
    out_pitch = dw if out_pitch is None else out_pitch
    ai, offi = VA.make_input(src, pitch, fs, off, "random", seed=seed)
    bo, go = VA.make_output(n, dh, dw, out_pitch, out_fs, out_off, seed=seed + 1)
    d_i, d_o = torch.from_numpy(ai).cuda(), torch.from_numpy(bo).cuda()
    torch.cuda.synchronize()
    ctx.pyr_down_device(d_i.data_ptr() + offi, pitch, pitch * h if fs is None else fs, w, h, d_o.data_ptr() + go.offset, out_pitch, go.frame_stride, n)
    ctx.sync()
    want = np.stack([R.pyr_down(src[f]) for f in range(n)])
    VA.check_output(d_o.cpu().numpy(), bo, go, want, f"pyr_down {w}x{h}x{n} in(pitch {pitch}, off {off}) out(pitch {out_pitch}, off {out_off})")
    assert np.array_equal(d_i.cpu().numpy(), ai), "the source arena changed"


PYR_SHAPES = [(3, 3), (5, 4), (63, 17), (64, 16), (65, 33), (257, 9), (130, 70)]
# A wave owns 248 source columns (lanes 1 .. 62; lanes 0 and 63 are halo), a work item 32 destination rows = 64 source rows.
# Widths 246 .. 254: the right border within 2 columns of the first strip's last lanes, of its halo lane 63, and of the second
# strip's first lanes (the edge lanes that gather bytewise, with a reflected column) -- at heights 3 .. 6, the smallest there are
PYR_SHAPES += [(w, h) for w in range(246, 255) for h in (3, 4, 5, 6)]
# ... the same at the seam between the second and the third strip; heights 63 .. 66: the bottom reflection (source rows h .. h + 1
# map to h - 2, h - 3) in the last rows of the first chunk and in the first rows -- the warm-up -- of the second
PYR_SHAPES += [(496, 3), (497, 65)] + [(33, h) for h in (63, 64, 65, 66)]
# ... and 2 strips x 2 chunks, 3 strips x 3 chunks: with n = 3 frames all three factors of the item decode exceed 1 at once
PYR_SHAPES += [(250, 66), (497, 130)]


@pytest.mark.parametrize("w,h", PYR_SHAPES)
def test_pyr_down_shapes_and_views(w, h):
    """Tight views with 1 and 3 frames; pitched, offset (every alignment of both sides) and ROI views; all in a context larger than
    the planes (a level of its frame)."""
    rng = np.random.default_rng(w * 1000 + h)
    dw = (w + 1) // 2
    with api.Context(w + 8, h + 2, 1, 3, api.MODE_O) as ctx:
        for n in (1, 3):
            src = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
            _pyr(ctx, src, seed=n)
            for k, (off, ooff) in enumerate([(1, 0), (2, 1), (3, 3), (4, 2)]):
                _pyr(ctx, src, pitch=w + 5 + k, fs=(w + 5 + k) * (h + 1) + k, off=off, out_pitch=dw + 3 + k, out_fs=(dw + 3 + k) * ((h + 1) // 2 + 2) + 1, out_off=ooff, seed=10 * n + k)
        src = np.stack([synth.natural(w, h, 5), np.full((h, w), 255, np.uint8), np.zeros((h, w), np.uint8)])
        _pyr(ctx, src, pitch=2 * w + 16, off=w // 2 + 4, out_pitch=w + 8, out_off=5, seed=77)  # ROIs of wider planes


def test_pyr_down_refusals_write_nothing():
    import torch
    with api.Context(64, 48, 1, 2, api.MODE_O) as ctx:
        src = torch.zeros(64 * 48 * 2, dtype=torch.uint8, device="cuda")
        dst = torch.full((32 * 24 * 2,), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        calls = [(src.data_ptr(), 64, 64 * 48, 2, 48, dst.data_ptr(), 32, 32 * 24, 1), (src.data_ptr(), 64, 64 * 48, 65, 48, dst.data_ptr(), 33, 33 * 24, 1),
                 (src.data_ptr(), 64, 64 * 48, 64, 48, dst.data_ptr(), 31, 32 * 24, 1), (src.data_ptr(), 64, 64 * 48, 64, 48, dst.data_ptr(), 32, 32 * 24, 3),
                 (src.data_ptr(), 64, 64 * 48, 64, 48, src.data_ptr() + 64, 32, 32 * 24, 1), (0, 64, 64 * 48, 64, 48, dst.data_ptr(), 32, 32 * 24, 1)]
        for c in calls:
            with pytest.raises(api.HipCannyError):
                ctx.pyr_down_device(*c)
        ctx.sync()
        assert bool((dst == 7).all()) and bool((src == 0).all())


# ---- one level of the tracker --------------------------------------------------------------------------------------------------
VIEW_KINDS = ("tight", "pitched", "stride", "ring", "side")


def _image_arena(prev, nxt, kind="tight", seed=0):
    """prev, nxt [n, h, w] in ONE arena of seeded random bytes: (arena, offset of prev, offset of next, pitch, frame stride).  The
    padding between rows and frames is random, so a kernel that walked rows by the width, or frames by height * pitch, would read
    other pixels than the reference.
      tight    rows of w, frames of w * h, next behind prev
      pitched  pitch w + 5, both bases odd
      stride   the frame stride exceeds h * pitch by 7
      ring     next is the frame after prev in one ring of n + 1 frames: d_next = d_prev + fs (nxt[f] must be prev[f + 1])
      side     prev and next are two ROIs side by side in the rows of one wider plane"""
    n, h, w = prev.shape
    if kind == "tight":
        pitch, fs, po = w, w * h, 0
        no = n * fs
    elif kind == "pitched":
        pitch, po = w + 5, 3
        fs = pitch * h
        no = (po + n * fs + 4) | 1
    elif kind == "stride":
        pitch, po = w + 2, 2
        fs = pitch * h + 7
        no = po + n * fs + 3
    elif kind == "ring":
        pitch, po = w + 3, 1
        fs = pitch * h + 5
        no = po + fs
        assert np.array_equal(nxt[:-1], prev[1:])
    elif kind == "side":
        pitch, po, no = 2 * w + 11, 2, w + 6
        fs = pitch * h + 1
    else:
        raise ValueError(kind)
    arena = np.random.default_rng(1000 + seed).integers(0, 256, max(po, no) + (n - 1) * fs + (h - 1) * pitch + w + 16, dtype=np.uint8)
    rows = lambda off: np.lib.stride_tricks.as_strided(arena[off:], (n, h, w), (fs, pitch, 1))
    rows(po)[...] = prev
    rows(no)[...] = nxt
    assert np.array_equal(rows(po), prev) and np.array_equal(rows(no), nxt), f"the views of kind {kind} do not hold both images"
    return arena, po, no, pitch, fs


class _Flow:
    """The point arrays of hc_lk_flow_device calls, each between guard words, on the device; status and err start from a pattern.
    call() queues one call on images wherever they are; check() compares everything with the reference's run on host copies of those
    images: next_pts and err as uint32 words, status as bytes, the guards, the slots beyond the counts, the input arrays."""
    G = 8

    def __init__(self, counts, prev_pts, start, with_err=True):
        import torch
        self.n, self.cap = prev_pts.shape[:2]
        self.counts, self.prev_pts, self.start, self.with_err = counts, prev_pts, start, with_err
        self.st0 = np.random.default_rng(1).integers(2, 250, (self.n, self.cap), dtype=np.uint8)
        self.er0 = np.full((self.n, self.cap), 123.5, np.float32)
        self.h_cnt, self.h_pp, self.h_np, self.h_er, self.h_st = self.pad32(np.asarray(counts, np.uint32)), self.pad32(prev_pts), self.pad32(start), self.pad32(self.er0), self.pad8(self.st0)
        self.d_cnt, self.d_pp, self.d_np, self.d_er = (torch.from_numpy(v.view(np.int32)).cuda() for v in (self.h_cnt, self.h_pp, self.h_np, self.h_er))
        self.d_st = torch.from_numpy(self.h_st).cuda()

    def pad32(self, a):
        return np.concatenate([np.full(self.G, GUARD, np.uint32), np.ascontiguousarray(a).view(np.uint32).reshape(-1), np.full(self.G, GUARD, np.uint32)])

    def pad8(self, a):
        return np.concatenate([np.full(4 * self.G, 0xA5, np.uint8), a.reshape(-1), np.full(4 * self.G, 0xA5, np.uint8)])

    def call(self, ctx, d_prev, d_next, pitch, fs, w, h, level, win, iters, eps, thr, use_initial):
        o = 4 * self.G
        self.args = (level, win, iters, eps, thr, use_initial)
        ctx.lk_flow_device(d_prev, d_next, pitch, fs, w, h, level, self.n, self.d_cnt.data_ptr() + o, self.d_pp.data_ptr() + o, self.d_np.data_ptr() + o, self.cap, win, iters,
                           eps, thr, use_initial, self.d_st.data_ptr() + o, self.d_er.data_ptr() + o if self.with_err else None)

    def check(self, prev, nxt, what=""):
        """(the reference's next_pts, its status, the device's next_pts words)"""
        G = self.G
        level, win, iters, eps, thr, use_initial = self.args
        w_np, w_st, w_er = R.lk_level(prev, nxt, level, self.counts, self.prev_pts, self.start, win, iters, eps, thr, use_initial, self.st0, self.er0 if self.with_err else None)
        n, h, w = prev.shape
        what = f"{what} {w}x{h}x{n} level {level} win {win} iterations {iters} eps {eps} initial {use_initial} counts {list(self.counts)}"
        g_np = self.d_np.cpu().numpy().view(np.uint32)
        bad = np.flatnonzero(g_np != self.pad32(w_np))
        assert bad.size == 0, f"{what}: next_pts words differ first at {bad[:6] - G}: got {g_np[bad[:6]].view(np.float32)} want {self.pad32(w_np)[bad[:6]].view(np.float32)}"
        g_st = self.d_st.cpu().numpy()
        bad = np.flatnonzero(g_st != self.pad8(w_st))
        assert bad.size == 0, f"{what}: status differs first at {bad[:6] - 4 * G}: got {g_st[bad[:6]]} want {self.pad8(w_st)[bad[:6]]}"
        g_er = self.d_er.cpu().numpy().view(np.uint32)
        bad = np.flatnonzero(g_er != self.pad32(w_er if self.with_err else self.er0))
        assert bad.size == 0, f"{what}: err words differ first at {bad[:6] - G}: got {g_er[bad[:6]].view(np.float32)}"
        assert np.array_equal(self.d_cnt.cpu().numpy().view(np.uint32), self.h_cnt) and np.array_equal(self.d_pp.cpu().numpy().view(np.uint32), self.h_pp), what + ": an input array changed"
        return w_np, w_st, g_np


def _level(ctx, prev, nxt, level, counts, prev_pts, start, win, iters, eps, thr, use_initial, with_err=True, what="", view="tight"):
    """One hc_lk_flow_device call with guard words around every array and the images in one arena of random bytes (view: a kind of
    _image_arena); everything is compared with the reference, and the arena whole with what it held.  prev, nxt [n, h, w];
    prev_pts, start [n, cap, 2].  Returns (the reference's next_pts, its status, the device's next_pts words)."""
    import torch
    n, h, w = prev.shape
    arena, po, no, pitch, fs = _image_arena(prev, nxt, view, seed=w + h + win)
    flow = _Flow(counts, prev_pts, start, with_err)
    d_arena = torch.from_numpy(arena).cuda()
    torch.cuda.synchronize()
    flow.call(ctx, d_arena.data_ptr() + po, d_arena.data_ptr() + no, pitch, fs, w, h, level, win, iters, eps, thr, use_initial)
    ctx.sync()
    out = flow.check(prev, nxt, f"{what} view {view} (pitch {pitch}, frame stride {fs}, offsets {po} / {no})")
    assert np.array_equal(d_arena.cpu().numpy(), arena), f"{what} view {view}: the arena of the images changed"
    return out


_pair, _points = FC.pair, FC.points


@pytest.mark.parametrize("win", [5, 7, 21, 31])
@pytest.mark.parametrize("w,h", [(48, 40), (97, 61)])
def test_flow_points_everywhere(w, h, win):
    a, b, pts, rng = FC.everywhere(w, h, win, win + w)
    if win == 5:
        flat = R.lk_point(a, b, 0, pts[-1], pts[-1], win, 30, 0.01, 1e-4, 0)
        assert flat[1] == 0 and np.array_equal(flat[0], pts[-1])
    cap = len(pts)
    with api.Context(w, h, 1, 3, api.MODE_O) as ctx:
        for iters, eps, init in [(30, 0.01, 0), (1, 0.01, 0), (30, 0.0, 1)]:
            start = (pts + rng.uniform(-1.5, 1.5, pts.shape).astype(np.float32))[None]
            _, st, _ = _level(ctx, a[None], b[None], 0, [cap], pts[None], start, win, iters, eps, 1e-4, init, with_err=(iters == 30))
            assert 0 < int(st.sum()) < cap


@pytest.mark.parametrize("win", FC.WINDOWS)
def test_flow_every_window(win):
    """All 14 windows -- the six compiled kernels k_lk_flow<1|2|4|7|10|16>, and in <4>, <7>, <10> and <16> the windows that leave
    whole rounds idle -- on one 48 x 40 frame, narrower than the largest windows reach from any point: borders, the out-of-frame
    rule, NaN, far away, a flat region; with and without the guess, with and without err, 30 and 2 iterations.
    test_flow_ref_cpu.py asserts that the reference tracks, loses (both ways) and iterates at every window."""
    a, b, pts, starts = FC.window_case(win)
    cap = len(pts)
    with api.Context(FC.WIN_W, FC.WIN_H, 1, 1, api.MODE_O) as ctx:
        for (iters, eps, init, with_err), start in zip(FC.WIN_RUNS, starts):
            _, st, _ = _level(ctx, a[None], b[None], 0, [cap], pts[None], start[None], win, iters, eps, 1e-4, init, with_err=with_err, what=f"kernel <{FC.flow_round_class(win)}>")
            assert 0 < int(st.sum()) < cap


@pytest.mark.parametrize("win", FC.TINY_WINDOWS)
@pytest.mark.parametrize("w,h", FC.TINY_SHAPES)
def test_flow_planes_smaller_than_the_window(w, h, win):
    """1 x 1, 1 x 9, 9 x 1 and 6 x 5 planes in a 48 x 40 context: every fetch but a few is clamped.  The first three are lost-only
    cases (no gradient in one direction at least: the reference loses every point, and next_pts keeps its start bit for bit); 6 x 5
    has tracked points at both windows."""
    a, b, pts = FC.tiny_case(w, h, win)
    with api.Context(48, 40, 1, 1, api.MODE_O) as ctx:
        for init in (0, 1):
            _, st, _ = _level(ctx, a[None], b[None], 0, [len(pts)], pts[None], (pts + np.float32(0.5))[None], win, 30, 0.01, 1e-4, init)
            assert (int(st.sum()) >= 3) if (w, h) == (6, 5) else not st.any()


def test_flow_level_15():
    """The scales 2^-15 and 2^15 (built from exponent bits): a 12 x 10 plane as level 15 of a 48 x 40 context, prev_pts in level-0
    units; tracked and lost points both (test_flow_ref_cpu.py); status and err keep their patterns."""
    a, b, pts, start = FC.top_level_case()
    with api.Context(48, 40, 1, 1, api.MODE_O) as ctx:
        for init in (0, 1):
            w_np, _, _ = _level(ctx, a[None], b[None], FC.TOP_LEVEL, [len(pts)], pts[None], start[None], FC.TOP_WIN, 30, 0.01, 1e-4, init)
            kept = (w_np.view(np.uint32) == (start if init else pts)[None].view(np.uint32)).all(axis=2)
            assert 0 < int(kept.sum()) < len(pts)


def test_flow_64_iterations():
    """max_iterations 64 with epsilon 0 on a pair where the reference runs all 64 for several points (test_flow_ref_cpu.py)."""
    a, b, pts = FC.long_case()
    with api.Context(FC.LONG_W, FC.LONG_H, 1, 1, api.MODE_O) as ctx:
        _, st, _ = _level(ctx, a[None], b[None], 0, [len(pts)], pts[None], np.zeros((1, len(pts), 2), np.float32), FC.LONG_WIN, 64, 0.0, 1e-4, 0)
        assert st.any()


@pytest.mark.parametrize("kind", VIEW_KINDS[1:])
def test_flow_views(kind):
    """n = 3 frames on pitched and offset views, a frame stride beyond height * pitch, `next` as the frame after `prev` in one ring
    and both as ROIs of one wider plane -- all in arenas of random bytes that are compared whole afterwards."""
    w, h, n, cap, win = 61, 37, 3, 10, 9
    ring = np.stack([synth.natural(w, h, 50), *[np.roll(synth.natural(w, h, 50), (k, 2 * k), (0, 1)) for k in (1, 2, 3)]])
    a, b = ring[:n], ring[1:]
    rng = np.random.default_rng(len(kind))
    pts = rng.uniform([3, 3], [w - 3, h - 3], (n, cap, 2)).astype(np.float32)
    pts[:, 0] = (0.25, h - 1.5)   # the clamped fetches of the first column and the last rows
    pts[:, 1] = (w - 1.25, 0.5)
    with api.Context(w + 3, h + 2, 1, n, api.MODE_O) as ctx:
        for init in (0, 1):
            _, st, _ = _level(ctx, a, b, 0, [cap, cap - 3, cap], pts, pts + np.float32([0.75, -0.5]), win, 30, 0.01, 1e-4, init, with_err=bool(init), view=kind)
            assert all(int(st[f].sum()) > 0 for f in range(n))


def test_flow_level_1_on_a_pitched_view():
    """Level-1 planes (48 x 40) of a 96 x 80 context on a pitched view with odd bases."""
    W, H, n = 96, 80, 3
    frames = [_pair(W, H, 60 + f, (2, -2 - 2 * f)) for f in range(n)]
    a, b = np.stack([R.pyr_down(f[0]) for f in frames]), np.stack([R.pyr_down(f[1]) for f in frames])
    pts = np.random.default_rng(1).uniform([4, 4], [W - 4, H - 4], (n, 8, 2)).astype(np.float32)
    with api.Context(W, H, 1, n, api.MODE_O) as ctx:
        for init in (0, 1):
            w_np, _, _ = _level(ctx, a, b, 1, [8, 8, 5], pts, pts + np.float32([-3, 2]), 11, 30, 0.01, 1e-4, init, view="pitched")
            assert not np.array_equal(w_np, pts)


@pytest.mark.parametrize("roll", FC.BIG_ROLLS + FC.STRIPE_ROLLS + FC.ROW_ROLLS, ids=lambda r: f"roll{r[0]}_{r[1]}")
def test_flow_where_32_bit_sums_wrap(roll):
    """The high dwords of wave_sum_i64: on 2 x 2 blocks of 0 / 255 the window sums of gx^2 and gy^2 reach 2^32 and those of
    diff * gx, diff * gy go beyond -2^31 (rolled by (1, 1)) and 2^31 (rolled by (-1, -1)) at windows 25 .. 31; on the stripes a
    sixteen-lane part of the sum leaves int32 by itself (vertical stripes, rolled by (0, +-1)), and an eight-lane part -- the only
    value beyond int32 that crosses lanes as two DPP moves -- does (horizontal stripes at window 31, rolled by (+-1, 0)).  Every
    such point is tracked (test_flow_ref_cpu.py), so a lost carry, a swapped half or a dropped high dword moves next_pts."""
    make, windows = ((FC.big_sum_case, FC.BIG_WINDOWS) if roll in FC.BIG_ROLLS else (FC.stripe_sum_case, FC.STRIPE_WINDOWS) if roll in FC.STRIPE_ROLLS
                     else (FC.row_sum_case, (FC.ROW_WIN,)))
    a, b, pts = make(roll)
    with api.Context(FC.BIG_W, FC.BIG_H, 1, 1, api.MODE_O) as ctx:
        for win in windows:
            _, st, _ = _level(ctx, a[None], b[None], 0, [len(pts)], pts[None], np.zeros((1, len(pts), 2), np.float32), win, 30, 0.01, 1e-4, 0)
            assert st.all()


@pytest.mark.parametrize("count_kind", ["zero", "one", "capacity", "beyond"])
def test_flow_counts_and_frames(count_kind):
    """counts of 0, 1, capacity and capacity + 5 in a batch of 3 frames with different counts; slots beyond min(count, capacity) are
    unchanged (the guards and the patterns of _level)."""
    w, h, cap = 48, 40, 9
    rng = np.random.default_rng(5)
    first = {"zero": 0, "one": 1, "capacity": cap, "beyond": cap + 5}[count_kind]
    frames = [_pair(w, h, s) for s in (1, 2, 3)]
    a, b = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    pts = rng.uniform([6, 6], [w - 6, h - 6], (3, cap, 2)).astype(np.float32)
    with api.Context(w, h, 1, 3, api.MODE_O) as ctx:
        _level(ctx, a, b, 0, [first, 4, cap - 1], pts, np.zeros_like(pts), 7, 30, 0.01, 1e-4, 0)
        _level(ctx, a[:1], b[:1], 0, [first], pts[:1], pts[:1] + np.float32(0.5), 7, 30, 0.01, 1e-4, 1, with_err=False)


def test_flow_half_step_stop():
    """The pair and points of the CPU search: synth.natural(48, 40, 0) rolled by (1, 2), epsilon 0, windows 5 and 7 -- the reference
    takes the 0.01 stop for several of these points, and the device agrees bit for bit."""
    a, b = _pair(48, 40, 0)
    rng = np.random.default_rng(0)
    pts = np.stack([rng.uniform([8, 8], [40, 32]).astype(np.float32) for _ in range(12)])
    with api.Context(48, 40, 1, 1, api.MODE_O) as ctx:
        for win in (5, 7):
            fired = [R.lk_point(a, b, 0, p, p, win, 30, 0.0, 1e-4, 0)[3]["half_step"] for p in pts]
            assert sum(fired) >= 2
            _level(ctx, a[None], b[None], 0, [12], pts[None], np.zeros((1, 12, 2), np.float32), win, 30, 0.0, 1e-4, 0)


@pytest.mark.parametrize("level", [0, 2])
def test_flow_levels_alone(level):
    """Levels 0 and 2 called alone on planes of that level in a context of the full frame; status and err are untouched at level 2
    (their start patterns are compared in _level)."""
    W, H = 192, 160
    a, b = _pair(W, H, 9, (4, -8))
    pa, pb = R.pyramid(a, level)[level], R.pyramid(b, level)[level]
    rng = np.random.default_rng(level)
    pts = rng.uniform([0, 0], [W, H], (1, 16, 2)).astype(np.float32)
    with api.Context(W, H, 1, 1, api.MODE_O) as ctx:
        for init in (0, 1):
            _level(ctx, pa[None], pb[None], level, [16], pts, pts + np.float32([-8, 4]), 9, 30, 0.01, 1e-4, init)


def test_flow_refusals_write_nothing():
    import torch
    w, h, cap = 48, 40, 4
    with api.Context(w, h, 1, 1, api.MODE_O) as ctx:
        img = torch.zeros((2, h, w), dtype=torch.uint8, device="cuda")
        cnt = torch.full((1,), cap, dtype=torch.int32, device="cuda")
        pp = torch.full((1, cap, 2), 20.0, dtype=torch.float32, device="cuda")
        np_ = torch.full((1, cap, 2), -1.0, dtype=torch.float32, device="cuda")
        st = torch.full((1, cap), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        good = dict(d_prev=img[0].data_ptr(), d_next=img[1].data_ptr(), pitch=w, fs=w * h, width=w, height=h, level=0, nframes=1, d_counts=cnt.data_ptr(), d_prev_pts=pp.data_ptr(),
                    d_next_pts=np_.data_ptr(), capacity=cap, win=7, max_iterations=10, epsilon=0.01, min_eig_threshold=1e-4, use_initial=0, d_status=st.data_ptr(), d_err=None)
        for change in [dict(win=6), dict(win=33), dict(win=3), dict(level=16), dict(level=-1), dict(max_iterations=0), dict(max_iterations=65), dict(epsilon=float("nan")),
                       dict(epsilon=-1.0), dict(min_eig_threshold=float("inf")), dict(capacity=0), dict(width=w + 1), dict(height=0), dict(nframes=2), dict(d_status=None),
                       dict(d_counts=None), dict(d_prev_pts=pp.data_ptr() + 2), dict(d_next_pts=pp.data_ptr()), dict(d_next_pts=cnt.data_ptr()), dict(d_next_pts=img[1].data_ptr()),
                       dict(pitch=w - 1)]:
            with pytest.raises(api.HipCannyError):
                ctx.lk_flow_device(**{**good, **change})
        ctx.sync()
        assert bool((np_ == -1.0).all()) and bool((st == 9).all())


# ---- behind pipelined runs, across stream switches, twice --------------------------------------------------------------------------
class _Pending:
    """The deterministic apparatus of tests/device_op_sequences.py without its model: a pipelined Mode R context of 130 x 67 that
    queues ONE hysteresis launch per run on 32-row tiles; the pool's first two frames hold a weak chain across the tiles
    (fuzz_sequences.vchain / wobble), so what a run's queued launch leaves differs from the final maps until finish_slot has continued
    the run from the host -- every time, not once in a while (test_gpu_device_op_sequences.py::test_the_neighbour_stays_in_flight
    reads that off the device for exactly these runs).  An entry that reads or writes a pending output without completing its run
    first therefore gives other words.  run(k, f0) queues the run of pool frames f0 .. f0 + 3 into output region k; the regions lie
    back to back in one tensor, full-size planes with rows of 132 bytes (the runs store dwords: 4-byte aligned views are written
    in place, as in the sequences)."""
    W, H, N, IP, OP = 130, 67, 4, 136, 132

    def __init__(self):
        import torch
        import device_op_sequences as DS
        w, h = self.W, self.H
        P = dict(w=w, h=h, ch=1, mode="R", per_channel=False, pool_kinds=["chain0", "chain1", "natural", "wobble", "natural", "sparse"], pool_seeds=[1, 2, 3, 4, 5, 6])
        self.frames = DS.pool_frames(P)
        self.ifs, self.fs = self.IP * h, self.OP * h
        self.region = self.N * self.fs
        self.ctx = api.Context(w, h, 1, self.N, api.MODE_R)
        self.ctx.set_thresholds(10, 40)
        self.ctx.set_option(api.OPT_PIPELINE, 1)
        self.ctx.set_option(api.OPT_TEST_HYST_GEOM, 1602)   # 32-row tiles
        self.ctx.set_tuning(0, 1)                           # one queued launch
        padded = np.zeros((len(self.frames), h, self.IP), np.uint8)
        padded[:, :, :w] = self.frames
        self.d_in = torch.from_numpy(padded).cuda()
        self.d_maps = torch.full((4 * self.region,), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ctx.close()

    def out(self, k, frame=0):
        return self.d_maps.data_ptr() + k * self.region + frame * self.fs

    def run(self, k, f0):
        self.ctx.run_device(self.d_in.data_ptr() + f0 * self.ifs, self.IP, self.ifs, self.out(k), self.OP, self.fs, self.N)

    def maps(self, k):
        """region k as the device holds it now, (4, H, W): torch's copy completes no run"""
        return np.ascontiguousarray(self.d_maps.cpu().numpy()[k * self.region:(k + 1) * self.region].reshape(self.N, self.H, self.OP)[:, :, :self.W])

    def continued(self):
        return self.ctx.hysteresis_totals()[1]

    def grid(self, n, step=5):
        gx, gy = np.meshgrid(np.arange(3, self.W - 2, step) + 0.5, np.arange(3, self.H - 3, step) + 0.25)
        return np.repeat(np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float32)[None], n, axis=0)


def test_pyr_down_of_a_pending_output():
    """Frames 1 .. 3 of a pipelined run's output, with the run in flight: the entry completes it first."""
    import torch
    with _Pending() as p:
        dw, dh = (p.W + 1) // 2, (p.H + 1) // 2
        dst = torch.zeros((3, dh, dw), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        p.run(0, 0)
        p.run(1, 1)
        p.ctx.pyr_down_device(p.out(0, 1), p.OP, p.fs, p.W, p.H, dst.data_ptr(), dw, dw * dh, 3)
        p.ctx.sync()
        final = p.maps(0)
        assert final[1].any() and np.array_equal(dst.cpu().numpy(), np.stack([R.pyr_down(final[f]) for f in (1, 2, 3)]))
        assert p.continued() == 2, "the runs were not continued from the host: their maps were final before the entry read them"


def test_pyr_down_into_a_pending_output():
    """Into the upper left quarters of frames 0 and 1 of a pending output: a run continued only afterwards would rewrite its whole
    maps over the planes."""
    with _Pending() as p:
        dw, dh = (p.W + 1) // 2, (p.H + 1) // 2
        p.run(2, 0)
        p.ctx.sync()
        final = p.maps(2)                 # what the run of frames 0 .. 3 leaves when it is complete
        assert p.continued() == 1
        p.run(0, 0)
        p.ctx.pyr_down_device(p.d_in.data_ptr() + 2 * p.ifs, p.IP, p.ifs, p.W, p.H, p.out(0), p.OP, p.fs, 2)
        p.ctx.sync()
        want = final.copy()
        for f in (0, 1):
            want[f, :dh, :dw] = R.pyr_down(p.frames[2 + f])
        got = p.maps(0)
        assert np.array_equal(got[:, :dh, :dw], want[:, :dh, :dw]), "the planes written into the pending output"
        assert np.array_equal(got, want), "the maps around the planes"
        assert p.continued() == 2


def test_flow_between_two_pending_outputs_and_not_a_run():
    """prev in one pending output, next in another, four frames and a grid of points over the whole frames; expected from the maps
    read back after the final sync.  Then the same call and a pyr_down again, complete: neither is a run (the schedule, the run info
    and the hysteresis info stay), and both give the same words."""
    import ctypes as C
    import torch
    with _Pending() as p:
        ctx, n = p.ctx, p.N
        pts = p.grid(n)
        cap = pts.shape[1]
        flow = _Flow([cap] * n, pts, np.zeros_like(pts))
        torch.cuda.synchronize()
        p.run(0, 0)
        p.run(1, 1)
        flow.call(ctx, p.out(0), p.out(1), p.OP, p.fs, p.W, p.H, 0, 9, 10, 0.01, 1e-4, 0)
        ctx.sync()
        prev, nxt = p.maps(0), p.maps(1)
        _, st, words = flow.check(prev, nxt, "prev and next in pending outputs")
        assert all(st[f].any() and not st[f].all() for f in range(n))
        assert p.continued() == 2, "the runs were not continued from the host"
        info = (C.c_int * len(api.SCHEDULE_FIELDS))()
        ri = [C.c_int(-5) for _ in range(3)]

        def state():
            assert ctx.lib.hc_last_hysteresis_schedule(ctx.handle, info, len(info)) >= 0
            assert ctx.lib.hc_last_run_info(ctx.handle, *[C.byref(v) for v in ri]) == 0
            return list(info), [v.value for v in ri], ctx.hysteresis_info(), ctx.hysteresis_totals()
        before = state()
        again = _Flow([cap] * n, pts, np.zeros_like(pts))
        dw, dh = (p.W + 1) // 2, (p.H + 1) // 2
        dst = torch.zeros((n, dh, dw), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        again.call(ctx, p.out(0), p.out(1), p.OP, p.fs, p.W, p.H, 0, 9, 10, 0.01, 1e-4, 0)
        ctx.pyr_down_device(p.out(1), p.OP, p.fs, p.W, p.H, dst.data_ptr(), dw, dw * dh, n)
        ctx.sync()
        assert state() == before
        assert np.array_equal(again.check(prev, nxt, "the same call again")[2], words)
        assert np.array_equal(dst.cpu().numpy(), np.stack([R.pyr_down(m) for m in nxt]))
        assert np.array_equal(p.maps(0), prev) and np.array_equal(p.maps(1), nxt)


def test_runs_that_write_elsewhere_stay_in_flight():
    """Full-size level-0 planes between two pending outputs -- `prev` begins where the region of one ends, `next` ends with the very
    byte before the other begins (for such planes finish_writers_of's byte range is exact): both entries give right results and
    complete neither run.  What shows an unfinished run is its output: with the device idle it holds what the one queued launch
    left, which differs from the final maps until hc_sync continues the run."""
    import torch
    with _Pending() as p:
        ctx, R1, fs, op = p.ctx, p.region, p.fs, p.OP
        a, b = p.frames[2:4], p.frames[4:6]
        host = np.full(4 * R1, 0x5A, np.uint8)          # regions: 0 a pending output | 1 the images | 2 a pending output | 3 unused
        o_prev, o_next = R1, 2 * R1 - (fs + (p.H - 1) * op + p.W)
        for off, img in ((o_prev, a), (o_next, b)):
            np.lib.stride_tricks.as_strided(host[off:], (2, p.H, p.W), (fs, op, 1))[...] = img
        assert o_prev + fs + (p.H - 1) * op + p.W <= o_next
        p.d_maps.copy_(torch.from_numpy(host))
        dw, dh = (p.W + 1) // 2, (p.H + 1) // 2
        dst = torch.zeros((2, 2, dh, dw), dtype=torch.uint8, device="cuda")
        pts = p.grid(2, step=9)
        flow = _Flow([pts.shape[1]] * 2, pts, np.zeros_like(pts))
        torch.cuda.synchronize()
        p.run(0, 0)
        p.run(2, 1)
        base = p.d_maps.data_ptr()
        flow.call(ctx, base + o_prev, base + o_next, op, fs, p.W, p.H, 0, 7, 10, 0.01, 1e-4, 0)
        ctx.pyr_down_device(base + o_prev, op, fs, p.W, p.H, dst[0].data_ptr(), dw, dw * dh, 2)
        ctx.pyr_down_device(base + o_next, op, fs, p.W, p.H, dst[1].data_ptr(), dw, dw * dh, 2)
        torch.cuda.synchronize()   # the device, not the context: no run is completed by this
        left = [p.maps(k) for k in (0, 2)]
        ctx.sync()
        for k, m in zip((0, 2), left):
            assert not np.array_equal(m, p.maps(k)), f"output {k} already held its final maps: its run was completed, or its content needs no continuation"
        assert p.continued() == 2
        _, st, _ = flow.check(a, b, "between pending outputs")
        assert st.any()
        assert np.array_equal(dst.cpu().numpy(), np.stack([[R.pyr_down(m) for m in a], [R.pyr_down(m) for m in b]]))
        assert np.array_equal(p.d_maps.cpu().numpy()[R1:2 * R1], host[R1:2 * R1]), "the images between the outputs changed"


def test_stream_switches_inside_a_chain():
    """pyr_down on the context's own stream, the level-1 call that reads its planes on a caller's stream (hc_set_stream), the
    level-0 call that reads the level-1 points on the own stream again (hc_use_own_stream), no host wait in between; then two
    independent level calls on either side of a switch."""
    import torch
    W, H, n, cap = 130, 70, 2, 12
    frames = [_pair(W, H, 80 + f, (2, 3 + f)) for f in range(n)]
    a, b = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    pts = np.random.default_rng(8).uniform([4, 4], [W - 4, H - 4], (n, cap, 2)).astype(np.float32)
    counts = [cap, cap - 4]
    with api.Context(W, H, 1, n, api.MODE_O) as ctx:
        da, db, dp = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(pts).cuda()
        dc = torch.tensor(counts, dtype=torch.int32, device="cuda")
        nxt, st, err = dp.clone(), torch.zeros((n, cap), dtype=torch.uint8, device="cuda"), torch.zeros((n, cap), dtype=torch.float32, device="cuda")
        dw, dh = (W + 1) // 2, (H + 1) // 2
        la, lb = (torch.empty((n, dh, dw), dtype=torch.uint8, device="cuda") for _ in range(2))
        nxt2, st2 = dp.clone(), torch.zeros((n, cap), dtype=torch.uint8, device="cuda")
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        for src, dst in ((da, la), (db, lb)):
            ctx.pyr_down_device(src.data_ptr(), W, W * H, W, H, dst.data_ptr(), dw, dw * dh, n)
        ctx.set_stream(side.cuda_stream)
        ctx.lk_level(la, lb, 1, dc, dp, nxt, 9, 30, 0.01, 1e-4, False, st, err)
        ctx.use_own_stream()
        ctx.lk_level(da, db, 0, dc, dp, nxt, 9, 30, 0.01, 1e-4, True, st, err)
        ctx.set_stream(side.cuda_stream)
        ctx.lk_level(db, da, 0, dc, dp, nxt2, 7, 30, 0.01, 1e-4, False, st2, None)
        ctx.sync()
        ctx.use_own_stream()
        ctx.sync()
        torch.cuda.synchronize()
        want = R.optical_flow(a, b, pts, counts, win=9, levels=1)
        assert np.array_equal(la.cpu().numpy(), np.stack([R.pyr_down(f) for f in a]))
        assert np.array_equal(nxt.cpu().numpy().view(np.uint32), want[0].view(np.uint32)) and np.array_equal(st.cpu().numpy(), want[1])
        assert np.array_equal(err.cpu().numpy().view(np.uint32), want[2].view(np.uint32)) and want[1].sum() > 0
        back = R.lk_level(b, a, 0, counts, pts, pts, 7, 30, 0.01, 1e-4, 0, np.zeros((n, cap), np.uint8))
        assert np.array_equal(nxt2.cpu().numpy().view(np.uint32), back[0].view(np.uint32)) and np.array_equal(st2.cpu().numpy(), back[1]) and back[1].sum() > 0


def test_repeatable():
    """The same level call and the same pyr_down twice on one context: equal words (the sums are integers, no atomics)."""
    import torch
    a, b, pts = FC.big_sum_case((1, 1))
    src = np.stack([synth.natural(497, 130, 7), synth.noise(497, 130, 8)])
    with api.Context(497, 130, 1, 2, api.MODE_O) as ctx:
        words = [_level(ctx, a[None], b[None], 0, [len(pts)], pts[None], np.zeros((1, len(pts), 2), np.float32), 31, 30, 0.0, 1e-4, 0, view="pitched")[2] for _ in range(2)]
        assert np.array_equal(words[0], words[1])
        d = torch.from_numpy(src).cuda()
        outs = [torch.zeros((2, 65, 249), dtype=torch.uint8, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        for o in outs:
            ctx.pyr_down_device(d.data_ptr(), 497, 497 * 130, 497, 130, o.data_ptr(), 249, 249 * 65, 2)
        ctx.sync()
        assert torch.equal(outs[0], outs[1]) and np.array_equal(outs[0].cpu().numpy()[0], R.pyr_down(src[0]))


# ---- the Python chains -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [0, 1, 3])
def test_optical_flow_chain(levels):
    W, H, n, cap = 130, 70, 2, 12
    frames = [_pair(W, H, 20 + f, (1 + f, 3)) for f in range(n)]
    a, b = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    rng = np.random.default_rng(levels)
    pts = rng.uniform([4, 4], [W - 4, H - 4], (n, cap, 2)).astype(np.float32)
    counts = [cap, cap - 5]
    with api.Context(W, H, 1, n, api.MODE_O) as ctx:
        for initial in (None, pts + np.float32([2.5, 1.0])):
            got = [t.cpu().numpy() for t in ctx.optical_flow(a, b, pts, counts, win=9, levels=levels, initial=initial)]
            want = R.optical_flow(a, b, pts, counts, win=9, levels=levels, initial=initial)
            assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))
            assert want[1].sum() > 0


def test_optical_flow_stops_the_pyramid_early():
    """20 x 9 with levels = 5: Context.optical_flow must stop at 5 x 3 -- a fourth plane would be 3 x 2, which hc_pyr_down_device
    refuses -- and track from level 2 down (test_flow_ref_cpu.py: the reference pyramid has 3 planes)."""
    a, b, pts, counts = FC.stop_case()
    with api.Context(FC.STOP_W, FC.STOP_H, 1, 2, api.MODE_O) as ctx:
        got = [t.cpu().numpy() for t in ctx.optical_flow(a, b, pts, counts, win=FC.STOP_WIN, levels=FC.STOP_LEVELS)]
        want = R.optical_flow(a, b, pts, counts, win=FC.STOP_WIN, levels=FC.STOP_LEVELS)
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))
        assert want[1].sum() > 0


def test_pyr_down_python():
    a = synth.natural(130, 70, 3)
    with api.Context(130, 70, 1, 1, api.MODE_O) as ctx:
        l1 = ctx.pyr_down(a)
        l2 = ctx.pyr_down(l1, width=65, height=35)
        assert np.array_equal(l1.cpu().numpy()[0], R.pyr_down(a)) and np.array_equal(l2.cpu().numpy()[0], R.pyr_down(R.pyr_down(a)))
        with pytest.raises(api.HipCannyError):
            ctx.pyr_down(a, width=64)


def test_track_end_to_end():
    """Detection and flow chained on the stream against the chained references: one seeded natural frame and its shifted copy."""
    import corner_ref as CR
    W, H, cap = 130, 70, 40
    a, b = _pair(W, H, 31, (2, 3))
    with api.Context(W, H, 1, 1, api.MODE_O) as ctx:
        counts, pts, nxt, status, err = (t.cpu().numpy() for t in ctx.track(a, b, max_corners=cap, min_distance=6, win=11, levels=2))
        dx, dy = ctx.derivatives(a, 3)
    resp = CR.corner_response(dx[0], dy[0], 3, CR.MIN_EIGEN, 0.04)
    cnt, xy, _ = CR.good_features(resp, 0.01, 6, 4096)
    m = min(cnt, cap)
    assert m > 5 and int(counts[0]) == m and np.array_equal(pts[0, :m], xy[:m]) and not pts[0, m:].any()
    want = R.optical_flow(a[None], b[None], pts, [m], win=11, levels=2)
    assert np.array_equal(nxt[0, :m].view(np.uint32), want[0][0, :m].view(np.uint32)) and not nxt[0, m:].any()
    assert np.array_equal(status, want[1]) and np.array_equal(err.view(np.uint32), want[2].view(np.uint32))
    assert (status[0, :m] == 1).any()
