"""hc_pyr_down_device (k_pyr_down8) and hc_lk_flow_device (k_lk_flow) on the MI355X, bit for bit against tests/flow_ref.py (anchored
by tests/test_flow_ref_cpu.py): planes compared as bytes, points as their uint32 words, status and err exactly.  The pyramid calls go
through guarded arenas (tests/view_arena.py): every byte around the destination rows is compared with what it held before.  The flow
calls put guard words around every array.  Sizes at lane, dword and strip seams; every window class; points at the borders, at the
out-of-frame rule, on flat content and NaN; counts below, at and above the capacity; the half-step stop; levels alone; the Python
chains."""
import numpy as np
import pytest

from cudacam_amd import api, synth
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
def _level(ctx, prev, nxt, level, counts, prev_pts, start, win, iters, eps, thr, use_initial, with_err=True, what=""):
    """One hc_lk_flow_device call with guard words around every array; everything is compared with the reference.  prev, nxt
    [n, h, w]; prev_pts, start [n, cap, 2]; the status and err arrays start from a pattern.  Returns the reference's next_pts."""
    import torch
    n, h, w = prev.shape
    cap = prev_pts.shape[1]
    G = 8
    st0 = np.random.default_rng(1).integers(2, 250, (n, cap), dtype=np.uint8)
    er0 = np.full((n, cap), 123.5, np.float32)
    pad32 = lambda a: np.concatenate([np.full(G, GUARD, np.uint32), np.ascontiguousarray(a).view(np.uint32).reshape(-1), np.full(G, GUARD, np.uint32)])
    pad8 = lambda a: np.concatenate([np.full(4 * G, 0xA5, np.uint8), a.reshape(-1), np.full(4 * G, 0xA5, np.uint8)])
    h_cnt, h_pp, h_np, h_er, h_st = pad32(np.asarray(counts, np.uint32)), pad32(prev_pts), pad32(start), pad32(er0), pad8(st0)
    d_a, d_b = torch.from_numpy(prev).cuda(), torch.from_numpy(nxt).cuda()
    d_cnt, d_pp, d_np, d_er = (torch.from_numpy(v.view(np.int32)).cuda() for v in (h_cnt, h_pp, h_np, h_er))
    d_st = torch.from_numpy(h_st).cuda()
    torch.cuda.synchronize()
    ctx.lk_flow_device(d_a.data_ptr(), d_b.data_ptr(), w, w * h, w, h, level, n, d_cnt.data_ptr() + 4 * G, d_pp.data_ptr() + 4 * G, d_np.data_ptr() + 4 * G, cap, win, iters,
                       eps, thr, use_initial, d_st.data_ptr() + 4 * G, d_er.data_ptr() + 4 * G if with_err else None)
    ctx.sync()
    w_np, w_st, w_er = R.lk_level(prev, nxt, level, counts, prev_pts, start, win, iters, eps, thr, use_initial, st0, er0 if with_err else None)
    what = f"{what} {w}x{h}x{n} level {level} win {win} iterations {iters} eps {eps} initial {use_initial} counts {list(counts)}"
    g_np = d_np.cpu().numpy().view(np.uint32)
    bad = np.flatnonzero(g_np != pad32(w_np))
    assert bad.size == 0, f"{what}: next_pts words differ first at {bad[:6] - G}: got {g_np[bad[:6]].view(np.float32)} want {pad32(w_np)[bad[:6]].view(np.float32)}"
    g_st = d_st.cpu().numpy()
    bad = np.flatnonzero(g_st != pad8(w_st))
    assert bad.size == 0, f"{what}: status differs first at {bad[:6] - 4 * G}: got {g_st[bad[:6]]} want {pad8(w_st)[bad[:6]]}"
    g_er = d_er.cpu().numpy().view(np.uint32)
    bad = np.flatnonzero(g_er != pad32(w_er if with_err else er0))
    assert bad.size == 0, f"{what}: err words differ first at {bad[:6] - G}: got {g_er[bad[:6]].view(np.float32)}"
    assert np.array_equal(d_cnt.cpu().numpy().view(np.uint32), h_cnt) and np.array_equal(d_pp.cpu().numpy().view(np.uint32), h_pp), what + ": an input array changed"
    assert np.array_equal(d_a.cpu().numpy(), prev) and np.array_equal(d_b.cpu().numpy(), nxt), what + ": an image changed"
    return w_np, w_st


def _pair(w, h, seed, shift=(1, 2)):
    a = synth.natural(w, h, seed)
    return a, np.ascontiguousarray(np.roll(a, shift, (0, 1)))


def _points(w, h, win, rng):
    """integer, half and arbitrary sub-pixel positions; within win of each border and each corner; exactly out of frame by the rule
    and just inside it; NaN; far away"""
    hw = (win - 1) * 0.5
    pts = [(w // 2, h // 2), (w // 2 + 0.5, h // 2 - 0.5), (w // 3 + 0.5, h // 3)]
    pts += [tuple(rng.uniform([4, 4], [w - 4, h - 4])) for _ in range(5)]
    pts += [(1.25, h / 2), (w - 1.5, h / 2), (w / 2, 0.75), (w / 2, h - 1.0), (0, 0), (w - 1, 0), (0.5, h - 1), (w - 1.25, h - 1.5), (win - 1.5, win - 2.25)]
    # the rule is on floor(p - hw): out at floor < -win and at floor >= w
    pts += [(hw - win - 0.25, h / 2), (hw - win, h / 2), (w + hw, h / 2), (w + hw - 0.25, h / 2), (w / 2, hw - win - 0.5), (w / 2, h + hw - 0.5), (w / 2, h + hw)]
    pts += [(np.nan, 5.0), (5.0, np.nan), (1e12, 3.0), (-3e9, 3.0), (np.inf, 1.0)]
    return np.float32(pts)


@pytest.mark.parametrize("win", [5, 7, 21, 31])
@pytest.mark.parametrize("w,h", [(48, 40), (97, 61)])
def test_flow_points_everywhere(w, h, win):
    rng = np.random.default_rng(win * 100 + w)
    a, b = _pair(w, h, win + w)
    a[h // 2 - 3:h // 2 + 8, 4:15] = 77   # a flat region: lost
    b[h // 2 - 3:h // 2 + 8, 4:15] = 77
    pts = np.concatenate([_points(w, h, win, rng), np.float32([[7.5, h // 2 + 1.25]])])
    if win == 5:
        flat = R.lk_point(a, b, 0, pts[-1], pts[-1], win, 30, 0.01, 1e-4, 0)
        assert flat[1] == 0 and np.array_equal(flat[0], pts[-1])
    cap = len(pts)
    with api.Context(w, h, 1, 3, api.MODE_O) as ctx:
        for iters, eps, init in [(30, 0.01, 0), (1, 0.01, 0), (30, 0.0, 1)]:
            start = (pts + rng.uniform(-1.5, 1.5, pts.shape).astype(np.float32))[None]
            _, st = _level(ctx, a[None], b[None], 0, [cap], pts[None], start, win, iters, eps, 1e-4, init, with_err=(iters == 30))
            assert 0 < int(st.sum()) < cap


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
