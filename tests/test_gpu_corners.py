"""hc_corner_response_device (k_corner_response) and hc_good_features_device (k_feat_*) on the MI355X through the C ABI, bit for
bit against tests/corner_ref.py (anchored by tests/test_corner_ref_cpu.py): float planes compared as bytes, corner lists, qualities
and counts exactly.  Every call goes through _response / _features: every buffer is a view of a guarded arena, and every byte of
every arena is compared -- the outputs with the reference, everything else with what it held before.
Shapes around the 4-pixel lane groups, the strip (CORNER_STRIP_W columns) and the row chunk (CORNER_CHUNK_ROWS rows) of
k_corner_response and around the trips (FEAT_TRIP_PX columns) and row groups (FEAT_GROUP_ROWS) of k_feat_plane; planes where 32-bit
sums wrap; hand-made response planes for the keys, the cut inside groups of equal keys, the interior rule and the distance rule;
caller views; passes under a small scratch bound; the refusals; chains with no synchronisation, also behind pipelined runs and
across a stream switch; the Python layer; repeatability."""
import os
import re

import numpy as np
import pytest

from cudacam_amd import api, synth
import corner_ref as R
import view_arena as VA

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _param(name):
    src = open(os.path.join(ROOT, "cudacam_amd", "csrc", "canny_params.h")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


STRIP, LANE_PX, CHUNK = _param("CORNER_STRIP_W"), _param("CORNER_LANE_PX"), _param("CORNER_CHUNK_ROWS")
TRIP, GROUP, BINS, STATE = _param("FEAT_TRIP_PX"), _param("FEAT_GROUP_ROWS"), _param("FEAT_BINS"), _param("FEAT_STATE_WORDS")
GUARD = 0xA5A5A5A5


def _lead(pitch, align=16):
    return VA.round_up(pitch + 64, align)   # the view's alignment is that of its base offset


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- one call of each entry on guarded arenas ------------------------------------------------------------------------------------
def _response(ctx, dx, dy, B, method, k=0.04, pitch=None, fs=None, off=0, out_pitch=None, out_fs=None, out_off=0, seed=0, what=""):
    """The corner measure of int16 planes [n, H, W]; checks everything and returns the float32 planes the device wrote."""
    import torch
    n, h, w = dx.shape
    pitch = 2 * w if pitch is None else pitch
    out_pitch = 4 * w if out_pitch is None else out_pitch
    ax, offx = VA.make_input(dx, pitch, fs, off, "random", lead=_lead(pitch), seed=seed)
    ay, offy = VA.make_input(dy, pitch, fs, off, "random", lead=_lead(pitch), seed=seed + 1)
    bo, go = VA.make_output(n, h, 4 * w, out_pitch, out_fs, out_off, lead=_lead(out_pitch), seed=seed + 2)
    d_x, d_y, d_o = (torch.from_numpy(v).cuda() for v in (ax, ay, bo))
    torch.cuda.synchronize()
    ctx.corner_response_device(d_x.data_ptr() + offx, d_y.data_ptr() + offy, pitch, pitch * h if fs is None else fs, d_o.data_ptr() + go.offset, out_pitch,
                               go.frame_stride, n, B, method, k)
    ctx.sync()
    want = np.stack([R.corner_response(dx[f], dy[f], B, method, k) for f in range(n)])
    what = f"{what} B {B} method {method} k {k} {w}x{h}x{n} in(pitch {pitch}, off {off}) out(pitch {out_pitch}, off {out_off})"
    after = d_o.cpu().numpy()
    VA.check_output(after, bo, go, want, what + ": response")
    assert np.array_equal(d_x.cpu().numpy(), ax) and np.array_equal(d_y.cpu().numpy(), ay), what + ": an input arena changed"
    return VA.read_view(after, go).reshape(n, h, 4 * w).view(np.float32)


def _features(ctx, planes, q, md, cc=4096, cap=None, quality=True, pitch=None, fs=None, off=0, seed=0, what=""):
    """good features of float32 planes [n, H, W]; checks everything and returns (counts, corners [n][cap][2], qualities [n][cap])."""
    import torch
    n, h, w = planes.shape
    pitch = 4 * w if pitch is None else pitch
    ap, offp = VA.make_input(planes, pitch, fs, off, "random", lead=_lead(pitch), seed=seed)
    ref = [R.good_features(planes[f], q, md, cc) for f in range(n)]
    cap = max(r[0] for r in ref) + 3 if cap is None else cap
    c0 = np.full(n + 8, GUARD, np.uint32)
    xy0 = np.full(2 * n * cap + 16, GUARD, np.uint32)
    q0 = np.full(n * cap + 8, GUARD, np.uint32)
    d_p, d_c, d_xy, d_q = (torch.from_numpy(v).cuda() for v in (ap, c0.view(np.int32), xy0.view(np.int32), q0.view(np.int32)))
    torch.cuda.synchronize()
    ctx.good_features_device(d_p.data_ptr() + offp, pitch, pitch * h if fs is None else fs, n, q, md, cc, d_c.data_ptr() + 16, d_xy.data_ptr() + 32 if cap else None,
                             d_q.data_ptr() + 16 if quality and cap else None, cap)
    ctx.sync()
    what = f"{what} q {q} min_distance {md} candidates {cc} capacity {cap} {w}x{h}x{n} (pitch {pitch}, off {off})"
    wc, wxy, wq = c0.copy(), xy0.copy(), q0.copy()
    for f, (cnt, xy, qual) in enumerate(ref):
        m = min(cnt, cap)
        wc[4 + f] = cnt
        wxy[8 + 2 * f * cap:8 + 2 * f * cap + 2 * m] = xy[:m].reshape(-1).view(np.uint32)
        if quality:
            wq[4 + f * cap:4 + f * cap + m] = qual[:m].view(np.uint32)
    gc, gxy, gq = (v.cpu().numpy().view(np.uint32) for v in (d_c, d_xy, d_q))
    assert np.array_equal(gc, wc), f"{what}: counts {gc[4:4 + n]} want {wc[4:4 + n]} (guards {gc[:4]} {gc[4 + n:]})"
    bad = np.flatnonzero(gxy != wxy)
    assert bad.size == 0, f"{what}: corner words differ first at {bad[:6] - 8}: got {gxy[bad[:6]].view(np.float32)} want {wxy[bad[:6]].view(np.float32)}"
    bad = np.flatnonzero(gq != wq)
    assert bad.size == 0, f"{what}: quality words differ first at {bad[:6] - 4}: got {gq[bad[:6]]} want {wq[bad[:6]]}"
    assert np.array_equal(d_p.cpu().numpy(), ap), what + ": the plane's arena changed"
    return gc[4:4 + n].copy(), gxy[8:8 + 2 * n * cap].view(np.float32).reshape(n, cap, 2) if cap else None, gq[4:4 + n * cap].view(np.float32).reshape(n, cap) if cap else None


def _int16_planes(rng, n, h, w, kind):
    if kind == "small":
        return tuple(rng.integers(-400, 400, (n, h, w)).astype(np.int16) for _ in range(2))
    return tuple(rng.integers(-32768, 32768, (n, h, w)).astype(np.int16) for _ in range(2))


# ---- the response ----------------------------------------------------------------------------------------------------------------
WIDTHS = sorted({1, 2, 3, LANE_PX - 1, LANE_PX, LANE_PX + 1, 2 * LANE_PX, 2 * LANE_PX + 1, STRIP - 1, STRIP, STRIP + 1, 2 * STRIP - 1, 2 * STRIP, 2 * STRIP + 1})


@pytest.mark.parametrize("B", [3, 5, 7])
@pytest.mark.parametrize("method", [R.MIN_EIGEN, R.HARRIS])
def test_response_widths_and_heights(B, method):
    """Widths at every lane-group and strip seam +- 1 and 1, 2, B - 1, B; heights 1, 2, B - 1, B, the ring length +- 1, the row chunk
    +- 1 and two chunks + 1."""
    rng = np.random.default_rng(10 * B + method)
    heights = sorted({1, 2, B - 1, B, B + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1})
    shapes = [(w, 9) for w in sorted(set(WIDTHS) | {B - 1, B})] + [(11, h) for h in heights] + [(STRIP + 1, CHUNK + 1), (2 * STRIP + 1, 2 * CHUNK + 1)]
    for i, (w, h) in enumerate(shapes):
        dx, dy = _int16_planes(rng, 2, h, w, "small" if i % 2 else "full")
        with api.Context(w, h, 1, 2, api.MODE_O) as ctx:
            _response(ctx, dx, dy, B, method, seed=i)


@pytest.mark.parametrize("ksize", [3, 5, 7, -1])
def test_response_of_device_derivatives(ksize):
    w, h = 300, 70
    frames = np.stack([synth.natural(w, h, 5), np.random.default_rng(ksize + 9).integers(0, 256, (h, w), dtype=np.uint8), (np.indices((h, w)).sum(0) % 23 < 9).astype(np.uint8) * 200])
    with api.Context(w, h, 1, 3, api.MODE_O) as ctx:
        dx, dy = ctx.derivatives(frames, ksize)
        for B, method in ((3, R.MIN_EIGEN), (5, R.HARRIS), (7, R.MIN_EIGEN), (7, R.HARRIS)):
            resp = _response(ctx, dx, dy, B, method, what=f"ksize {ksize}")
            assert (resp > 0).any()


def test_response_where_32_bit_sums_wrap():
    """Constant -32768, +-32767 checkerboards and random full-range int16 at B = 7: a reaches 49 * 2^30."""
    w, h = 53, 19
    yy, xx = np.indices((h, w))
    board = np.where((yy + xx) % 2 == 0, 32767, -32767).astype(np.int16)
    rng = np.random.default_rng(3)
    dx = np.stack([np.full((h, w), -32768, np.int16), board, -board, rng.integers(-32768, 32768, (h, w)).astype(np.int16)])
    dy = np.stack([np.full((h, w), -32768, np.int16), board, board, rng.integers(-32768, 32768, (h, w)).astype(np.int16)])
    assert int(R.window_sums(dx[0], dy[0], 7)[0].max()) == 49 << 30
    with api.Context(w, h, 1, 4, api.MODE_O) as ctx:
        for method in (R.MIN_EIGEN, R.HARRIS):
            for B in (3, 7):
                _response(ctx, dx, dy, B, method)


def test_response_single_pixels_on_the_border_and_harris_k():
    """One non-zero pixel at each corner and edge midpoint of the frame (the clamped window), at harris_k 0, 0.04, 0.25."""
    w, h = 2 * STRIP + 3, 9
    spots = [(y, x) for y in (0, h // 2, h - 1) for x in (0, w // 2, w - 1) if (y, x) != (h // 2, w // 2)]
    dx, dy = np.zeros((len(spots), h, w), np.int16), np.zeros((len(spots), h, w), np.int16)
    for f, (y, x) in enumerate(spots):
        dx[f, y, x], dy[f, y, x] = 1000 + f, -700 + 3 * f
    with api.Context(w, h, 1, len(spots), api.MODE_O) as ctx:
        for B in (3, 5, 7):
            _response(ctx, dx, dy, B, R.MIN_EIGEN)
            for k in (0.0, 0.04, 0.25):
                _response(ctx, dx, dy, B, R.HARRIS, k)


def test_response_views():
    """Pitched, offset and ROI views at every alignment class of either side; dx and dy in one plane's arena layout."""
    w, h, n = STRIP + 5, 13, 2
    dx, dy = _int16_planes(np.random.default_rng(4), n, h, w, "full")
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        for i, (pad, off, opad, ooff) in enumerate(((0, 0, 0, 0), (2, 2, 4, 4), (4, 4, 8, 8), (8, 8, 16, 16), (6, 10, 12, 20), (64, 0, 128, 0))):
            pitch, op = 2 * w + pad, 4 * w + opad
            _response(ctx, dx, dy, 5, R.HARRIS, 0.04, pitch, pitch * h + 3 * pad, off, op, op * h + 5 * opad, ooff, seed=i)
            _response(ctx, dx, dy, 3, R.MIN_EIGEN, 0.0, pitch, None, off, op, None, ooff, seed=i)


def test_response_refusals():
    import torch
    w, h, n = 40, 12, 2
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        x = torch.zeros(4 * n * h * (2 * w + 8), dtype=torch.uint8, device="cuda")
        o = torch.full((4 * n * h * (4 * w + 16),), 7, dtype=torch.uint8, device="cuda")
        X, Y, O = x.data_ptr(), x.data_ptr() + n * h * (2 * w + 8) + 64, o.data_ptr()
        torch.cuda.synchronize()
        ok = dict(d_dx=X, d_dy=Y, pitch=2 * w, fs=2 * w * h, d_response=O, out_pitch=4 * w, out_fs=4 * w * h, nframes=n, block_size=3, method=0, k=0.04)
        ctx.corner_response_device(**ok)
        cases = [(dict(d_dx=0), "null"), (dict(d_dy=0), "null"), (dict(d_response=0), "null"), (dict(d_dx=X + 1), "multiples"), (dict(pitch=2 * w + 1, fs=(2 * w + 1) * h), "multiples"),
                 (dict(d_response=O + 2), "multiples of 4"), (dict(out_pitch=4 * w + 2, out_fs=(4 * w + 2) * h), "multiples of 4"), (dict(pitch=2 * w - 2), "pitch smaller"), (dict(out_pitch=4 * w - 4), "pitch smaller"),
                 (dict(pitch=VA.round_up((1 << 32) // h + 1, 4), nframes=1), "2^32"), (dict(out_pitch=VA.round_up((1 << 32) // h + 1, 4), nframes=1), "2^32"), (dict(fs=2 * w * h - 2), "frame stride"),
                 (dict(out_fs=4 * w * h - 4), "frame stride"), (dict(block_size=4), "block_size"), (dict(block_size=9), "block_size"), (dict(method=2), "method"), (dict(method=-1), "method"),
                 (dict(method=1, k=float("nan")), "harris_k"), (dict(method=1, k=float("inf")), "harris_k"), (dict(nframes=0), "nframes"), (dict(nframes=n + 1), "nframes"),
                 (dict(d_response=X), "overlap"), (dict(d_response=Y + 2 * w * h * n - 4), "overlap"), (dict(d_dx=(1 << 64) - 64, nframes=1), "wraps"),
                 (dict(d_dy=(1 << 64) - 64, nframes=1), "wraps"), (dict(d_response=(1 << 64) - 64, nframes=1), "wraps")]
        for change, text in cases:
            with pytest.raises(api.HipCannyError, match=re.escape(text)):
                ctx.corner_response_device(**dict(ok, **change))
        ctx.corner_response_device(**dict(ok, method=0, k=float("nan")))   # ignored with MIN_EIGEN
        ctx.sync()
        assert bool((o[4 * w * h * n:] == 7).all()), "a refused call wrote"


# ---- the features: hand-made planes ----------------------------------------------------------------------------------------------
def _f32_from_bits(b):
    return np.asarray(b, np.uint32).view(np.float32)


def _isolated(h, w, values, step=2, y0=1, x0=1):
    """zeros with values[i] at the i-th position of a grid of pitch `step` from (y0, x0): every one a local maximum of its own"""
    p = np.zeros((h, w), np.float32)
    ys, xs = np.meshgrid(np.arange(y0, h - 1, step), np.arange(x0, w - 1, step), indexing="ij")
    m = min(len(values), ys.size)
    p[ys.reshape(-1)[:m], xs.reshape(-1)[:m]] = values[:m]
    return p


def test_features_special_values():
    """NaN, +-inf, -0, negatives and denormals: keys, the threshold product and the maximum."""
    h, w = 21, 2 * TRIP + 5
    rng = np.random.default_rng(11)
    pool = np.array([np.nan, -np.inf, -0.0, -3.0, 1e-41, 3e-39, 1.0, 2.5, 0.0], np.float32)
    dense = pool[rng.integers(0, len(pool), (h, w))]
    with_inf = dense.copy(); with_inf[7, 9] = np.inf
    tiny = _isolated(h, w, _f32_from_bits(rng.integers(1, 50, 400)))   # denormals only: t = M q is a denormal product
    planes = np.stack([dense, with_inf, tiny])
    with api.Context(w, h, 1, 3, api.MODE_O) as ctx:
        for q, md in ((0.01, 0.0), (0.5, 2.0), (1.0, 0.0)):
            cnt, _, _ = _features(ctx, planes, q, md)
            assert cnt[1] == 0   # M = +inf: nothing lies above t = inf
        assert _features(ctx, planes, 0.01, 0.0)[0][0] > 0


@pytest.mark.parametrize("cc", [1, 2, 64, 65, 4096])
def test_features_constant_plane_cut_by_index(cc):
    """A constant positive plane: every interior pixel a candidate, the cut is purely by index; N below, equal to and above 4096."""
    for (w, h) in ((66, 66), (40, 30), (130, 70)):   # 4096, 1064 and 8704 interior pixels
        plane = np.full((1, h, w), 3.25, np.float32)
        with api.Context(w, h, 1, 1, api.MODE_O) as ctx:
            cnt, xy, _ = _features(ctx, plane, 0.5, 0.0, cc, cap=min(cc, (w - 2) * (h - 2)) + 2)
            assert cnt[0] == min(cc, (w - 2) * (h - 2))
            _features(ctx, plane, 0.5, 1.5, cc)


@pytest.mark.parametrize("cc", [1, 2, 64, 65, 300])
def test_features_cut_inside_groups_of_equal_keys(cc):
    """Keys that differ only inside each digit of the select (11 + 11 + 10 bits) and across each digit boundary, many of each: the
    cut falls inside a group of equal keys, of which the first in raster order are admitted."""
    base = 0x3F800000
    levels = np.array([base, base + 1, base + 0x3FF, base + 0x400, base + 0x401, base + 0x1FFFFF, base + 0x200000, base + 0x200001, base + 0x200400], np.uint32)
    h, w = 2 * GROUP + 3, 2 * TRIP + 7
    rng = np.random.default_rng(cc)
    planes = []
    for nlev in (1, 3, len(levels)):
        vals = _f32_from_bits(levels[rng.integers(0, nlev, 2000)])
        planes.append(_isolated(h, w, vals))
    planes = np.stack(planes)
    for f in range(len(planes)):
        kk, _ = R.candidates(planes[f], 0.01)
        assert len(kk) > cc and kk[cc - 1] == kk[cc]   # the cut lies inside a tie
    with api.Context(w, h, 1, len(planes), api.MODE_O) as ctx:
        cnt, _, _ = _features(ctx, planes, 0.01, 0.0, cc)
        assert (cnt == cc).all()
        _features(ctx, planes, 0.01, 2.5, cc)


@pytest.mark.parametrize("digit", [0, 1, 2])
def test_features_cut_in_a_tie_group_below_larger_keys(digit):
    """The cut key T lies below keys that differ from it in ONE digit of the select only (digit 0: bits 21 .., digit 1: bits 10 ..
    20, digit 2: bits 0 .. 9), with smaller keys below it that differ in that digit too: the walk of that pass carries the
    candidates above its digit (`above`), the passes before it see one bin, the passes after it see the tie group alone."""
    base, step = 0x3F800000, (1 << 21, 1 << 10, 1)[digit]
    T = base + 5 * step
    h, w = 2 * GROUP + 3, 2 * TRIP + 7
    rng = np.random.default_rng(digit)
    keys = np.array([T + 2 * step] * 5 + [T + step] * 10 + [T] * 600 + [T - step] * 300 + [T - 3 * step] * 300, np.uint32)
    planes = np.stack([_isolated(h, w, _f32_from_bits(rng.permutation(keys))) for _ in range(2)])
    with api.Context(w, h, 1, 2, api.MODE_O) as ctx:
        for cc in (5, 6, 15, 16, 64, 65, 300, 615, 616, 1000):
            kk, _ = R.candidates(planes[0], 0.01)
            assert len(kk) == len(keys) and (cc not in (16, 64, 65, 300) or (kk[cc - 1] == T and kk[cc] == T and kk[0] > T))
            cnt, _, _ = _features(ctx, planes, 0.01, 0.0, cc, what=f"digit {digit}")
            assert (cnt == cc).all()
        _features(ctx, planes, 0.01, 2.5, 300, what=f"digit {digit}")


def test_features_tie_group_at_4096():
    """More than 4096 candidates, a hundred above T and the rest equal to it: the cut at candidate_capacity 4096 and 4095 falls
    inside the tie group."""
    h, w = 2 * GROUP + 3, 4 * TRIP + 11
    T = 0x3F800400
    keys = np.array([T + 1] * 60 + [T + 0x400] * 40 + [T] * 4150, np.uint32)
    plane = _isolated(h, w, _f32_from_bits(np.random.default_rng(4096).permutation(keys)))[None]
    kk, _ = R.candidates(plane[0], 0.01)
    assert len(kk) == len(keys) > 4096 and kk[4095] == T == kk[4096] and kk[99] > T
    with api.Context(w, h, 1, 1, api.MODE_O) as ctx:
        for cc in (4096, 4095):
            cnt, _, _ = _features(ctx, plane, 0.01, 0.0, cc)
            assert cnt[0] == cc


def test_features_interior_rule_and_border_maximum():
    """Maxima on the interior's first and last row and column and on the outermost ones: the outermost count for M and as
    neighbours, never as corners.  A frame whose M sits on the border only.  An all-zero frame between two busy ones."""
    h, w = GROUP + 5, TRIP + 9
    a = np.zeros((h, w), np.float32)
    for i, (y, x) in enumerate([(0, 5), (1, 9), (h - 2, 13), (h - 1, 17), (5, 0), (9, 1), (13, w - 2), (17, w - 1), (0, 0), (h - 1, w - 1), (1, 1), (h - 2, w - 2), (10, 10)]):
        a[y, x] = 5.0 + i
    b = _isolated(h, w, np.full(300, 1.0, np.float32), step=3, y0=1, x0=1)
    b[0, 4] = 100.0   # the maximum, on the border; (1, 4) is a peak beside it
    planes = np.stack([a, np.zeros((h, w), np.float32), b])
    with api.Context(w, h, 1, 3, api.MODE_O) as ctx:
        cnt, xy, _ = _features(ctx, planes, 0.001, 0.0)   # (t = 0.017 and 0.1: every peak passes)
        got = {(int(x), int(y)) for x, y in xy[0][:cnt[0]]}
        assert got == {(9, 1), (13, h - 2), (1, 9), (w - 2, 13), (1, 1), (w - 2, h - 2), (10, 10)} and cnt[1] == 0 and cnt[2] > 0
        cnt, _, _ = _features(ctx, planes, 0.5, 0.0)
        assert cnt[2] == 0   # t = 50: no interior pixel passes
        _features(ctx, planes, 0.005, 3.0)


@pytest.mark.parametrize("w, h", [(2, 10), (10, 2), (1, 1), (3, 3), (TRIP + 2, 3), (TRIP + 3, 4)])
def test_features_small_frames(w, h):
    plane = np.random.default_rng(w * h).random((2, h, w)).astype(np.float32)
    with api.Context(w, h, 1, 2, api.MODE_O) as ctx:
        cnt, _, _ = _features(ctx, plane, 0.01, 0.0)
        assert (w >= 3 and h >= 3) or not cnt.any()


def test_features_distance_rule():
    """Pairs of equal-key and unequal-key maxima at squared distance min_d2 - 1, min_d2 and min_d2 + 1; min_distance 0; a distance
    larger than the frame leaves one corner."""
    h, w = 30, 40
    planes = []
    for (ddx, ddy) in ((2, 2), (0, 3), (1, 3)):   # 8, 9, 10 against min_d2 = 9
        for second in (7.0, 6.0):
            p = np.zeros((h, w), np.float32)
            p[10, 12], p[10 + ddy, 12 + ddx] = 7.0, second
            planes.append(p)
    planes = np.stack(planes)
    assert R.min_d2(3.0) == 9
    with api.Context(w, h, 1, len(planes), api.MODE_O) as ctx:
        cnt, _, _ = _features(ctx, planes, 0.01, 3.0)
        assert cnt.tolist() == [1, 1, 2, 2, 2, 2]
        assert _features(ctx, planes, 0.01, 0.0)[0].tolist() == [2] * 6
        assert _features(ctx, planes, 0.01, 1000.0)[0].tolist() == [1] * 6
        assert _features(ctx, planes, 0.01, 1e300)[0].tolist() == [1] * 6


def test_features_capacities_quality_and_views():
    """corner_capacity 0, below and above the count; d_quality null and given; pitched, offset and ROI views of the plane."""
    h, w, n = GROUP + 3, 2 * TRIP + 1, 3
    rng = np.random.default_rng(21)
    planes = rng.random((n, h, w)).astype(np.float32)
    planes[1] = np.round(planes[1] * 4) / 4   # plateaus
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        full = _features(ctx, planes, 0.05, 2.0)[0]
        assert full.min() > 8
        for cap in (0, 1, int(full.min()) - 1, int(full.max()) + 5):
            for quality in (True, False):
                _features(ctx, planes, 0.05, 2.0, cap=cap, quality=quality)
        for i, (pad, off) in enumerate(((4, 4), (12, 8), (64, 20))):
            pitch = 4 * w + pad
            _features(ctx, planes, 0.05, 2.0, 100, pitch=pitch, fs=pitch * h + 8 * pad, off=off, seed=i)
            _features(ctx, planes, 0.3, 0.0, 4096, pitch=pitch, off=off, seed=i)


def test_features_passes_under_a_small_scratch_bound():
    h, w, n, cc = 20, 50, 5, 64
    planes = np.random.default_rng(5).random((n, h, w)).astype(np.float32)
    planes[2] = 0
    frame = 40 * cc + 4 * BINS + 4 * STATE + 8 * h
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        for bound in (5 * frame, 3 * frame, 2 * frame, 2 * frame - 1, frame):
            ctx.set_option(api.OPT_TEST_HOUGH_SCRATCH, bound)
            _features(ctx, planes, 0.1, 3.0, cc, what=f"bound {bound}")
        ctx.set_option(api.OPT_TEST_HOUGH_SCRATCH, frame - 1)
        with pytest.raises(api.HipCannyError, match="scratch bound"):
            _features(ctx, planes, 0.1, 3.0, cc)
        ctx.set_option(api.OPT_TEST_HOUGH_SCRATCH, 0)
        _features(ctx, planes, 0.1, 3.0, 4096)


def test_features_refusals():
    import torch
    w, h, n = 40, 12, 2
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        p = torch.ones((n, h, w), dtype=torch.float32, device="cuda")
        c = torch.full((16,), 7, dtype=torch.int32, device="cuda")
        xy = torch.full((n * 8 * 2 + 16,), 7, dtype=torch.int32, device="cuda")
        ql = torch.full((n * 8 + 16,), 7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ok = dict(d_response=p.data_ptr(), pitch=4 * w, fs=4 * w * h, nframes=n, quality_level=0.01, min_distance=1.0, candidate_capacity=4096, d_corner_counts=c.data_ptr(),
                  d_corners=xy.data_ptr(), d_quality=ql.data_ptr(), corner_capacity=8)
        cases = [(dict(d_response=0), "null"), (dict(d_corner_counts=0), "null"), (dict(d_corners=0), "d_corners is null"), (dict(d_response=p.data_ptr() + 2), "multiples of 4"),
                 (dict(pitch=4 * w + 2, fs=(4 * w + 2) * h), "multiples of 4"), (dict(d_corner_counts=c.data_ptr() + 2), "d_corner_counts"), (dict(d_corners=xy.data_ptr() + 4), "d_corners must be 8"),
                 (dict(d_quality=ql.data_ptr() + 2), "d_quality"), (dict(pitch=4 * w - 4), "pitch smaller"), (dict(pitch=VA.round_up((1 << 32) // h + 1, 4), nframes=1), "2^32"),
                 (dict(fs=4 * w * h - 4), "frame stride"), (dict(quality_level=0.0), "quality_level"), (dict(quality_level=1.5), "quality_level"), (dict(quality_level=float("nan")), "quality_level"),
                 (dict(min_distance=-1.0), "min_distance"), (dict(min_distance=float("inf")), "min_distance"), (dict(candidate_capacity=0), "candidate_capacity"),
                 (dict(candidate_capacity=4097), "candidate_capacity"), (dict(nframes=0), "nframes"), (dict(nframes=n + 1), "nframes"), (dict(corner_capacity=(1 << 64) // 16 + 1), "overflows"),
                 (dict(d_response=(1 << 64) - 64, nframes=1), "wraps")]
        for change, text in cases:
            with pytest.raises(api.HipCannyError, match=re.escape(text)):
                ctx.good_features_device(**dict(ok, **change))
        ctx.sync()
        assert bool((c == 7).all()) and bool((xy == 7).all()) and bool((ql == 7).all()), "a refused call wrote"
        ctx.good_features_device(**dict(ok, d_corners=0, d_quality=0, corner_capacity=0))
        ctx.sync()
        assert c.cpu().numpy()[:n].tolist() == [R.good_features(np.ones((h, w), np.float32), 0.01, 1.0)[0]] * n


# ---- chains ----------------------------------------------------------------------------------------------------------------------
def _chain_buffers(d_frames, n, w, h, blur, cap):
    """the device tensors of one chain: (source or blurred source, dx, dy, response, counts, corners, qualities)"""
    import torch
    src = d_frames if blur is None else torch.empty_like(d_frames)
    gx, gy = torch.empty((n, h, w), dtype=torch.int16, device="cuda"), torch.empty((n, h, w), dtype=torch.int16, device="cuda")
    resp = torch.empty((n, h, w), dtype=torch.float32, device="cuda")
    counts = torch.zeros((n,), dtype=torch.int32, device="cuda")
    xy = torch.zeros((n, cap, 2), dtype=torch.float32, device="cuda")
    ql = torch.zeros((n, cap), dtype=torch.float32, device="cuda")
    return src, gx, gy, resp, counts, xy, ql


def _chain_queue(ctx, d_frames, t, n, w, h, ksize, B, method, blur, q, md, cap):
    """blur -> derivatives -> response -> features queued on the context stream: no host wait of any kind in here"""
    src, gx, gy, resp, counts, xy, ql = t
    fs = w * h
    if blur is not None:
        ctx.gaussian_blur_device(d_frames.data_ptr(), w, fs, src.data_ptr(), w, fs, n, blur[0], api.gaussian_taps_q8(*blur))
    ctx.derivatives_device(src.data_ptr(), w, fs, gx.data_ptr(), gy.data_ptr(), 2 * w, 2 * fs, n, ksize)
    ctx.corner_response_device(gx.data_ptr(), gy.data_ptr(), 2 * w, 2 * fs, resp.data_ptr(), 4 * w, 4 * fs, n, B, method, 0.04)
    ctx.good_features_device(resp.data_ptr(), 4 * w, 4 * fs, n, q, md, 4096, counts.data_ptr(), xy.data_ptr(), ql.data_ptr(), cap)


def _chain(ctx, d_frames, n, w, h, ksize, B, method, blur, q, md, cap):
    """the buffers (torch's stream waited for once), then the four entries queued with no synchronisation; the device tensors"""
    import torch
    t = _chain_buffers(d_frames, n, w, h, blur, cap)
    torch.cuda.synchronize()
    _chain_queue(ctx, d_frames, t, n, w, h, ksize, B, method, blur, q, md, cap)
    return t


def _check_chain(ctx, frames, tensors, ksize, B, method, blur, q, md, cap, what):
    src, gx, gy, resp, counts, xy, ql = (t.cpu().numpy() for t in tensors)
    n = len(frames)
    blurred = frames if blur is None else ctx.gaussian_blur(frames, *blur)
    wx, wy = ctx.derivatives(blurred, ksize)
    assert np.array_equal(src, blurred) and np.array_equal(gx, wx) and np.array_equal(gy, wy), what + ": blur / derivatives"
    for f in range(n):
        want = R.corner_response(gx[f], gy[f], B, method, 0.04)
        assert np.array_equal(_bits(resp[f]), _bits(want)), what + ": response"
        cnt, wxy, wq = R.good_features(want, q, md, 4096, cap)
        assert int(counts.view(np.uint32)[f]) == cnt and cnt > 3, what
        assert np.array_equal(xy[f, :len(wxy)], wxy) and np.array_equal(_bits(ql[f, :len(wq)]), _bits(wq)), what + ": corners"


def test_chain_blur_derivatives_response_features():
    import torch
    w, h, n = 320, 100, 2
    frames = np.stack([synth.natural(w, h, 40 + i) for i in range(n)])
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        d = torch.from_numpy(frames).cuda()
        for ksize, B, method, blur in ((3, 3, R.MIN_EIGEN, (5, 1.2)), (5, 5, R.HARRIS, None), (-1, 7, R.MIN_EIGEN, (3, 0.0))):
            t = _chain(ctx, d, n, w, h, ksize, B, method, blur, 0.02, 6.0, 500)
            ctx.sync()
            _check_chain(ctx, frames, t, ksize, B, method, blur, 0.02, 6.0, 500, f"chain ksize {ksize} B {B}")


def test_chain_behind_pipelined_runs_and_not_a_run():
    import torch
    w, h, n = 256, 96, 2
    sets = [np.stack([synth.natural(w, h, 70 + 10 * i + j) for j in range(n)]) for i in range(3)]
    fs = w * h
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        ctx.set_thresholds(40, 90)
        ctx.set_option(api.OPT_PIPELINE, 1)
        srcs = [torch.from_numpy(s).cuda() for s in sets]
        outs = [torch.empty_like(s) for s in srcs]
        torch.cuda.synchronize()
        for s, o in zip(srcs, outs):
            ctx.run_device(s.data_ptr(), w, fs, o.data_ptr(), w, fs, n)
        t = _chain(ctx, srcs[1], n, w, h, 3, 5, R.HARRIS, (3, 0.8), 0.02, 4.0, 300)
        ctx.sync()
        _check_chain(ctx, sets[1], t, 3, 5, R.HARRIS, (3, 0.8), 0.02, 4.0, 300, "behind pipelined runs")
        assert all(bool(o.any()) for o in outs)
        before = (ctx.last_run_info(), ctx.hysteresis_info())
        t = _chain(ctx, srcs[2], n, w, h, 3, 3, R.MIN_EIGEN, None, 0.02, 4.0, 300)
        ctx.sync()
        assert (ctx.last_run_info(), ctx.hysteresis_info()) == before   # not a run
        _check_chain(ctx, sets[2], t, 3, 3, R.MIN_EIGEN, None, 0.02, 4.0, 300, "after the runs")


def test_chain_across_a_stream_switch():
    """Three whole chains -- on the context's own stream, on a caller's stream (hc_set_stream) and on its own again
    (hc_use_own_stream) -- queued with no host wait between them: the features scratch is shared across both switches."""
    import torch
    w, h, n = 200, 60, 3
    sets = [np.stack([synth.natural(w, h, 300 + 10 * i + j) for j in range(n)]) for i in range(3)]
    cases = ((3, 3, R.MIN_EIGEN, (3, 0.0), 0.05, 5.0, 64), (5, 5, R.HARRIS, None, 0.02, 3.0, 100), (3, 7, R.MIN_EIGEN, None, 0.1, 4.0, 80))
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        srcs = [torch.from_numpy(f).cuda() for f in sets]
        bufs = [_chain_buffers(d, n, w, h, c[3], c[6]) for d, c in zip(srcs, cases)]
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        _chain_queue(ctx, srcs[0], bufs[0], n, w, h, *cases[0])
        ctx.set_stream(s.cuda_stream)
        _chain_queue(ctx, srcs[1], bufs[1], n, w, h, *cases[1])
        ctx.use_own_stream()
        _chain_queue(ctx, srcs[2], bufs[2], n, w, h, *cases[2])
        ctx.sync()
        torch.cuda.synchronize()
        for i, (frames, t, c) in enumerate(zip(sets, bufs, cases)):
            _check_chain(ctx, frames, t, *c, f"chain {i} across the stream switches")


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
def test_python_layer():
    w, h, n = 180, 70, 2
    frames = np.stack([synth.natural(w, h, 90 + i) for i in range(n)])
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        dx, dy = ctx.derivatives(frames, 3)
        resp = ctx.corner_response(dx, dy, 5, "harris", 0.06).cpu().numpy()
        want = np.stack([R.corner_response(dx[f], dy[f], 5, R.HARRIS, 0.06) for f in range(n)])
        assert np.array_equal(_bits(resp), _bits(want))
        one = ctx.corner_response(dx[0], dy[0]).cpu().numpy()
        assert np.array_equal(_bits(one[0]), _bits(R.corner_response(dx[0], dy[0], 3, R.MIN_EIGEN)))
        with pytest.raises(api.HipCannyError):
            ctx.corner_response(dx, dy, 3, "fast")
        xy, ql = ctx.good_features(want, 0.05, 5.0, max_corners=20)
        for f in range(n):
            cnt, wxy, wq = R.good_features(want[f], 0.05, 5.0, 4096, 20)
            assert np.array_equal(xy[f], wxy) and np.array_equal(_bits(ql[f]), _bits(wq))
        xy_all, _ = ctx.good_features(want[0], 0.05, 5.0)
        assert len(xy_all[0]) == R.good_features(want[0], 0.05, 5.0)[0]
        xy, ql = ctx.features(frames, ksize=3, block_size=3, method="min_eigen", quality_level=0.01, min_distance=10, max_corners=50, blur=(3, 0.0))
        blurred = ctx.gaussian_blur(frames, 3, 0.0)
        bx, by = ctx.derivatives(blurred, 3)
        for f in range(n):
            cnt, wxy, wq = R.good_features(R.corner_response(bx[f], by[f], 3, R.MIN_EIGEN), 0.01, 10, 4096, 50)
            assert len(wxy) > 5 and np.array_equal(xy[f], wxy) and np.array_equal(_bits(ql[f]), _bits(wq))
    with api.Context(w, h, 3, 1, api.MODE_O) as ctx3:
        with pytest.raises(ValueError):
            ctx3.features(np.zeros((1, h, w, 3), np.uint8))


def test_repeatable():
    w, h, n = 2 * STRIP + 9, CHUNK + 7, 2
    dx, dy = _int16_planes(np.random.default_rng(77), n, h, w, "full")
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        r1 = _response(ctx, dx, dy, 7, R.HARRIS)
        r2 = _response(ctx, dx, dy, 7, R.HARRIS)
        assert np.array_equal(_bits(r1), _bits(r2))
        noise = np.abs(r1) / np.float32(1e18)
        f1 = _features(ctx, noise, 0.001, 2.0, 1000, cap=1000)
        f2 = _features(ctx, noise, 0.001, 2.0, 1000, cap=1000)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(f1, f2))
