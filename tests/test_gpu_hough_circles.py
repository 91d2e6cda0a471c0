"""hc_hough_circles_device (k_circle_vote, the peaks of hough.hip, k_circle_rank, k_circle_sift, k_circle_radii, k_circle_scan) on
the MI355X: circle counts and circles equal, value for value, bit for bit in the floats and in order, to the numpy restatement
tests/hough_circles_ref.py.  Every call writes its counts between two guard words and its circles into a buffer pre-filled with a
canary with guard space on both sides -- everything but the first min(count, circle_capacity) circles of each frame's slot must
still hold the canary -- and reads points, counts and gradient planes (inside arenas of random bytes) that must come back unchanged.

The sizes are the smallest at which the paths differ: accumulator rows shorter than, equal to and longer than a wave, point lists
around one wave and beyond one workgroup trip, histograms of 1, 60 .. 65 and more than 256 bins (a bin is a radius: max_radius -
min_radius + 1 of them, two words more in the kernel's table), so that the radius rule's last trip of 64 radii is full, one short
and one over, and the table ends at, before and behind word 64.

No vacuous passes: each parametrised drawn case asserts, on the restatement alone, that its input has at least two circles, a
centre dropped by min_dist, a centre with two radii, a ray cut by the accumulator's border and a tie in the votes.  Two
exceptions, each stated where it is made: a 9 x 7 frame cannot hold all of these and has a test of its own, and a histogram of
one bin gives no centre two radii."""
import math

import numpy as np
import pytest

import hough_circles_ref as HC
import view_arena as VA
from cudacam_amd import api

pytestmark = pytest.mark.gpu

CANARY = -0x5A5A5A5B
GUARD = 64   # int32 words: 256 bytes, so the slots behind it keep the allocation's 16-byte alignment
SIZES = [(33, 31), (64, 48), (65, 64), (130, 67), (200, 150)]
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def _scene(w, h, seed, extra_points=0):
    """One frame: planes of random gradients (a share of them zero, some extreme) with circles drawn over them -- two concentric
    ones, one that leaves the frame, a small one -- and the point list: the perimeters, then random pixels.  Returns (points int32
    (k, 2), dx, dy)."""
    rng = np.random.default_rng(seed)
    dx = rng.integers(-400, 401, (h, w)).astype(np.int16)
    dy = rng.integers(-400, 401, (h, w)).astype(np.int16)
    zero = rng.random((h, w)) < 0.2
    dx[zero], dy[zero] = 0, 0
    ext = rng.random((h, w)) < 0.02
    dx[ext] = rng.choice(np.array([-32768, 32767, 0, 1, -1], np.int16), int(ext.sum()))
    dy[ext] = rng.choice(np.array([-32768, 32767, 0, 1, -1], np.int16), int(ext.sum()))
    m = min(w, h)
    r1 = max(3, m // 6)
    pts = [HC.draw(dx, dy, w, h, w * 0.4, h * 0.45, r1), HC.draw(dx, dy, w, h, w * 0.4, h * 0.45, r1 + max(3, m // 8)),
           HC.draw(dx, dy, w, h, w - 2.0, h * 0.5, max(3, m // 5)), HC.draw(dx, dy, w, h, w * 0.75, h * 0.25, 3, strength=-30000)]
    k = w * h // 12 + extra_points
    pts.append(np.stack([rng.integers(0, w, k), rng.integers(0, h, k)], axis=1).astype(np.int32))
    return np.concatenate(pts), dx, dy


def _upload(points, counts, dx, dy, circle_capacity, point_capacity=None, pitch=None, frame_stride=None, base_off=0):
    """The buffers of one call: per-frame point lists (k_f, 2) padded to [n][pcap][2] with a poison coordinate, their counts, both
    planes [n, h, w] int16 inside arenas of random bytes, the circle counts between two guard words and the circle slots between
    guards, pre-filled with the canary.  point_capacity 0 is taken as given: the lists are [n][0][2], and d_points is a buffer of
    poison coordinates the entry has no reason to read."""
    import torch
    n, h, w = dx.shape
    pcap = max(1, max(len(p) for p in points)) if point_capacity is None else point_capacity
    lists = np.full((n, pcap, 2), 0x7F7F7F7F, np.int32)
    for f, p in enumerate(points):
        lists[f, :min(len(p), pcap)] = p[:pcap]
    on_device = lists if pcap else np.full((n, 64, 2), 0x7F7F7F7F, np.int32)
    pitch = pitch or 2 * w
    ax, off = VA.make_input(dx, pitch, frame_stride, base_off, fill="random", seed=1)
    ay, _ = VA.make_input(dy, pitch, frame_stride, base_off, fill="random", seed=2)
    g = VA.input_geometry(dx, pitch, frame_stride, base_off)
    counts = np.asarray(counts, np.uint32)
    return dict(n=n, w=w, h=h, lists=lists, on_device=on_device, pcounts=counts, pcap=pcap, dx=dx, dy=dy, ax=ax, ay=ay, off=off, g=g, cap=circle_capacity,
                d_pts=torch.from_numpy(on_device).cuda(), d_pc=torch.from_numpy(counts.view(np.int32)).cuda(), d_ax=torch.from_numpy(ax).cuda(), d_ay=torch.from_numpy(ay).cuda(),
                counts=torch.full((n + 2,), CANARY, dtype=torch.int32, device="cuda"),
                circles=torch.full((2 * GUARD + 4 * n * circle_capacity,), CANARY, dtype=torch.int32, device="cuda"))


def _queue(ctx, b, par, centre_capacity=4096, null_circles=False):
    ctx.hough_circles_device(b["d_pts"].data_ptr(), b["d_pc"].data_ptr(), b["pcap"], b["d_ax"].data_ptr() + b["off"], b["d_ay"].data_ptr() + b["off"], b["g"].pitch,
                             b["g"].frame_stride, b["n"], *par, centre_capacity, b["counts"].data_ptr() + 4, None if null_circles else b["circles"].data_ptr() + 4 * GUARD, b["cap"])


def _want(b, par, centre_capacity=4096, stats=None):
    used = [b["lists"][f, :min(int(b["pcounts"][f]), b["pcap"])] for f in range(b["n"])]
    dp, min_dist, thr, rmin, rmax = par
    return HC.circles_batch(used, b["dx"], b["dy"], b["w"], b["h"], dp, min_dist, thr, rmin, rmax, centre_capacity, b["cap"], stats)


def _check(b, par, centre_capacity=4096, what="", want=None):
    """What a call left behind (the context has been synchronised), compared with the restatement.  Returns (counts, circles)."""
    n, cap = b["n"], b["cap"]
    assert np.array_equal(b["d_ax"].cpu().numpy(), b["ax"]) and np.array_equal(b["d_ay"].cpu().numpy(), b["ay"]), f"{what}: a gradient plane or the bytes around it were written"
    assert np.array_equal(b["d_pts"].cpu().numpy(), b["on_device"]) and np.array_equal(b["d_pc"].cpu().numpy().view(np.uint32), b["pcounts"]), f"{what}: the points were written"
    c = b["counts"].cpu().numpy()
    assert c[0] == CANARY and c[-1] == CANARY, f"{what}: a word beside d_circle_counts was written"
    got_counts = c[1:-1].view(np.uint32)
    want_counts, want_circles = want or _want(b, par, centre_capacity)
    assert got_counts.tolist() == want_counts.tolist(), f"{what}: counts {got_counts.tolist()} != {want_counts.tolist()}"
    s = b["circles"].cpu().numpy()
    assert (s[:GUARD] == CANARY).all() and (s[len(s) - GUARD:] == CANARY).all(), f"{what}: the guard around d_circles was written"
    slots = s[GUARD:len(s) - GUARD].reshape(n, cap, 4)
    for f in range(n):
        k = len(want_circles[f])
        assert k == min(int(want_counts[f]), cap)
        w32 = want_circles[f].view(np.int32)
        if not np.array_equal(slots[f, :k], w32):
            bad = np.flatnonzero((slots[f, :k] != w32).any(axis=1))
            raise AssertionError(f"{what}: frame {f}: {len(bad)} of {k} circles differ; first (index, hip, numpy): "
                                 f"{[(int(i), slots[f, i].view(np.float32).tolist(), want_circles[f][i].tolist()) for i in bad[:6]]}")
        assert (slots[f, k:] == CANARY).all(), f"{what}: frame {f}: the slot was written behind its {k} circles"
    return got_counts, want_circles


def _call(ctx, points, dx, dy, par, circle_capacity, counts=None, centre_capacity=4096, null_circles=False, what="", **view):
    import torch
    b = _upload(points, [len(p) for p in points] if counts is None else counts, dx, dy, circle_capacity, **view)
    torch.cuda.synchronize()
    _queue(ctx, b, par, centre_capacity, null_circles)
    ctx.sync()
    return _check(b, par, centre_capacity, what)


def _not_vacuous(points, dx, dy, w, h, par, what, two_radii=True):
    """The conditions on an input, on the restatement alone.  two_radii=False: the one case that cannot hold a centre with two radii."""
    stats = {}
    dp, min_dist, thr, rmin, rmax = par
    HC.circles_of(points, dx, dy, w, h, dp, min_dist, thr, rmin, rmax, stats=stats)
    assert stats["circles"] >= 2 and stats["dropped"] > 0 and stats["cut_rays"] > 0 and stats["ties"] > 0 and (stats["two_radii"] > 0 or not two_radii), f"{what}: a vacuous input: {stats}"


def _params(w, h, dp):
    m = min(w, h)
    return (dp, 4.0, 3, 2, max(6, m // 2))   # dp, min_dist, votes_threshold, min_radius, max_radius


@pytest.mark.parametrize("dp", [1.0, 1.5, 2.0])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_size_and_dp(size, dp):
    w, h = size
    par = _params(w, h, dp)
    scenes = [_scene(w, h, 100 + k) for k in range(2)]
    for k, sc in enumerate(scenes):
        _not_vacuous(*sc, w, h, par, f"{w}x{h} dp {dp} scene {k}")
    pts = [s[0] for s in scenes] + [np.empty((0, 2), np.int32)]
    dx = np.stack([s[1] for s in scenes] + [scenes[0][1]])
    dy = np.stack([s[2] for s in scenes] + [scenes[0][2]])
    with api.Context(w, h, 1, 3, api.MODE_O if dp == 1.5 else api.MODE_R) as ctx:   # either mode
        t = f"{w}x{h} dp {dp}"
        counts, _ = _call(ctx, pts, dx, dy, par, 4096, what=t)
        assert counts[0] >= 2 and counts[2] == 0
        _call(ctx, pts, dx, dy, (dp, 0.0, 0, 1, par[4]), 64, what=t + " threshold 0, min_dist 0, cut lists")
        _call(ctx, pts[:1], dx[:1], dy[:1], par, 0, null_circles=True, what=t + " counts only")


def test_a_frame_of_9_by_7():
    """9 x 7: accumulators of 9 x 7, 6 x 5 and 5 x 4 cells; circles of radius 1.5 and 3 round one centre."""
    w, h = 9, 7
    dx, dy = np.zeros((h, w), np.int16), np.zeros((h, w), np.int16)
    pts = np.concatenate([HC.draw(dx, dy, w, h, 4, 3, 1.5), HC.draw(dx, dy, w, h, 4, 3, 3)])
    for dp in (1.0, 1.5, 2.0):
        par = (dp, 2.0, 1, 1, 4)
        stats = {}
        count, _ = HC.circles_of(pts, dx, dy, w, h, *par, stats=stats)
        assert count >= 2 and stats["cut_rays"] > 0, stats
        with api.Context(w, h, 1, 2) as ctx:
            counts, _ = _call(ctx, [pts, pts[::-1]], np.stack([dx, dx]), np.stack([dy, dy]), par, 100, what=f"9x7 dp {dp}")
            assert counts[0] == count


@pytest.mark.parametrize("npoints", [63, 64, 65, 300, 1000])
def test_point_lists_around_a_wave_and_a_workgroup(npoints):
    w, h = 64, 48
    p, dx, dy = _scene(w, h, 7, extra_points=1000)
    par = _params(w, h, 1.0)
    _not_vacuous(p[:npoints], dx, dy, w, h, par, f"{npoints} points")   # (the first 63 points are perimeter points of the concentric circles: all five conditions hold)
    with api.Context(w, h, 1, 1) as ctx:
        counts, _ = _call(ctx, [p[:npoints]], dx[None], dy[None], par, 1024, what=f"{npoints} points")
        assert counts[0] >= 2


@pytest.mark.parametrize("radii", [(5, 5), (3, 62), (3, 63), (3, 64), (3, 65), (3, 66), (3, 67), (2, 300), (1, 4094)], ids=lambda r: f"{r[0]}..{r[1]}")
def test_histograms_of_1_60_to_65_and_up_to_4094_bins(radii):
    """max_radius - min_radius + 1 bins: 1; 60 and 61 (tables of 62 and 63 words); 62 and 63 (tables of 64 and 65 words: the rule's
    hist[i + 2] reaches word 63, then word 64); 64 and 65 (one full trip of 64 radii, then a second trip with one live lane); 299
    and 4094 (the largest table).  Each of the cases up to 65 bins has, in the restatement, a circle of the largest radius: the last
    bin and the zero word behind it decide something.  One bin gives no centre two radii: that condition alone is not asked of it."""
    w, h = 130, 67
    p, dx, dy = _scene(w, h, 11)
    dp = 1.0
    if radii[0] == radii[1]:   # one bin counts rad == 5 exactly: twelve points on the integer circle round (41, 31), the centre of cell (20, 15) at dp 2
        dp = 2.0
        ring = np.array([(41 + a, 31 + b) for a, b in ((5, 0), (-5, 0), (0, 5), (0, -5), (3, 4), (3, -4), (-3, 4), (-3, -4), (4, 3), (4, -3), (-4, 3), (-4, -3))], np.int32)
        dx[ring[:, 1], ring[:, 0]], dy[ring[:, 1], ring[:, 0]] = 200 * (ring[:, 0] - 41), 200 * (ring[:, 1] - 31)
        p = np.concatenate([ring, p])
    par = (dp, 6.0, 2, *radii)
    count, circles = HC.circles_of(p, dx, dy, w, h, *par)
    assert count > 0 and count <= 8192
    _not_vacuous(p, dx, dy, w, h, par, f"radii {radii}", two_radii=radii[0] != radii[1])
    if radii[1] <= 67:
        assert (circles[:, 2] == radii[1]).any(), "no circle of the largest radius"
    with api.Context(w, h, 1, 1) as ctx:
        counts, _ = _call(ctx, [p], dx[None], dy[None], par, 8192, what=f"radii {radii}")   # (the capacity holds every circle: none of the largest radius is cut)
        assert counts[0] == count


def test_hostile_coordinates_take_part_in_nothing():
    """Coordinates outside the frame, negative, INT32_MIN / INT32_MAX, between the points of a scene: the result is that of the
    restatement, which drops them, and every canary is intact.  The contract says such points are skipped."""
    w, h = 65, 64
    p, dx, dy = _scene(w, h, 21)
    bad = np.array([(-1, 0), (0, -1), (w, 0), (0, h), (w, h), (I32_MIN, I32_MIN), (I32_MAX, I32_MAX), (I32_MIN, 5), (5, I32_MAX), (I32_MAX, 0), (0, I32_MIN),
                    (65536 + 3, 3), (3, 65536 + 3), (1 << 30, 1 << 30), (-(1 << 20), 7), (w - 1, h - 1), (0, 0)], np.int32)
    mixed = np.concatenate([bad, p[:200], bad[::-1], p[200:], bad])
    par = _params(w, h, 1.5)
    clean = HC.circles_of(p, dx, dy, w, h, *par)[0]
    with api.Context(w, h, 1, 2) as ctx:
        counts, _ = _call(ctx, [mixed, bad], np.stack([dx, dx]), np.stack([dy, dy]), par, 2048, what="hostile")
        assert clean > 0 and counts[0] > 0   # (the two in-frame corners of `bad` take part as well)


def test_cuts_by_every_capacity():
    w, h = 64, 48
    scenes = [_scene(w, h, 30 + k) for k in range(3)]
    par = _params(w, h, 1.0)
    _not_vacuous(*scenes[0], w, h, par, "capacities")
    pts = [s[0] for s in scenes] + [np.empty((0, 2), np.int32)]
    dx, dy = np.stack([s[1] for s in scenes] + [scenes[1][1]]), np.stack([s[2] for s in scenes] + [scenes[1][2]])
    c0 = HC.circles_of(*scenes[0], w, h, *par)[0]
    ncentres = len(HC.centres(HC.accumulate(*scenes[0], w, h, par[0], par[3], par[4]), par[2]))
    assert c0 > 3 and ncentres > 8
    with api.Context(w, h, 1, 4) as ctx:
        _call(ctx, pts, dx, dy, par, 0, null_circles=True, what="capacity 0, null")
        _call(ctx, pts, dx, dy, par, 0, what="capacity 0, a pointer")
        for cap in (1, c0 - 1, c0, c0 + 1):
            _call(ctx, pts, dx, dy, par, cap, what=f"circle_capacity {cap}")
        for cc in (1, 2, ncentres - 1, ncentres, ncentres + 1):
            _call(ctx, pts, dx, dy, par, 512, centre_capacity=cc, what=f"centre_capacity {cc}")
        for pcap in (1, 64, len(pts[0]) - 1):
            _call(ctx, pts, dx, dy, par, 512, point_capacity=pcap, what=f"point_capacity {pcap}")
        _call(ctx, pts, dx, dy, par, 512, counts=[len(pts[0]), 0xFFFFFFFF, 5, 0], point_capacity=len(pts[1]) + 3, what="counts beyond the capacity")


def test_point_capacity_0():
    """point_capacity 0 with a d_points that is not null: frame f uses its first min(d_point_counts[f], 0) points, whatever the
    counts say -- no circle, every slot untouched, and the call after it is none the worse."""
    import torch
    w, h = 64, 48
    scenes = [_scene(w, h, 30 + k) for k in range(2)]
    par = _params(w, h, 1.0)
    pts, dx, dy = [s[0] for s in scenes], np.stack([s[1] for s in scenes]), np.stack([s[2] for s in scenes])
    with api.Context(w, h, 1, 2) as ctx:
        for cap in (256, 0):
            b = _upload(pts, [len(pts[0]), 0xFFFFFFFF], dx, dy, cap, point_capacity=0)
            assert b["pcap"] == 0 and b["lists"].shape == (2, 0, 2) and b["d_pts"].data_ptr() % 8 == 0 and b["d_pts"].data_ptr() != 0
            torch.cuda.synchronize()
            _queue(ctx, b, par)
            ctx.sync()
            counts, circles = _check(b, par, what=f"point_capacity 0, circle_capacity {cap}")
            assert counts.tolist() == [0, 0] and [len(c) for c in circles] == [0, 0]
            assert (b["circles"].cpu().numpy() == CANARY).all()
        counts, _ = _call(ctx, pts, dx, dy, par, 256, what="a valid call after point_capacity 0")
        assert counts.min() > 0


def test_pitched_offset_roi_planes_and_passes():
    """Even base offsets, pitches and frame strides beyond the tight ones: every byte around the planes is random.  Then the same
    batch cut into passes of one and of two frames by a small scratch bound."""
    w, h, n = 65, 64, 3
    scenes = [_scene(w, h, 40 + k) for k in range(n)]
    par = _params(w, h, 1.5)
    pts, dx, dy = [s[0] for s in scenes], np.stack([s[1] for s in scenes]), np.stack([s[2] for s in scenes])
    with api.Context(w, h, 1, n) as ctx:
        tight, _ = _call(ctx, pts, dx, dy, par, 1024, what="tight")
        assert tight.min() > 0
        for pitch, extra, base in ((2 * w + 2, 0, 2), (262, 78, 14), (2 * w, 2, 6)):
            got, _ = _call(ctx, pts, dx, dy, par, 1024, what=f"pitch {pitch} base {base}", pitch=pitch, frame_stride=pitch * h + extra, base_off=base)
            assert got.tolist() == tight.tolist()
        aw, ah, _ = api.hough_circle_geometry(w, h, 1.5, 4.0, par[3], par[4])
        per_frame = 2 * 16 * 4096 + 8 * ah * ((aw + 1) // 2) + 4 * (ah + 2) * (aw + 2) + 4 * ah + 4 * 4096 + 8
        for frames in (1, 2):
            ctx.set_option(api.OPT_TEST_HOUGH_SCRATCH, frames * per_frame + 7)
            got, _ = _call(ctx, pts, dx, dy, par, 1024, what=f"passes of {frames}")
            assert got.tolist() == tight.tolist()
        ctx.set_option(api.OPT_TEST_HOUGH_SCRATCH, per_frame - 1)
        with pytest.raises(api.HipCannyError, match="scratch bound"):
            _call(ctx, pts, dx, dy, par, 1024)
        ctx.set_option(api.OPT_TEST_HOUGH_SCRATCH, 0)
        _call(ctx, pts, dx, dy, par, 1024, what="the default bound again")


def test_two_geometries_on_one_context_queued_back_to_back():
    import torch
    w, h = 130, 67
    p, dx, dy = _scene(w, h, 50)
    pars = [(2.0, 3.0, 2, 2, 12), (1.0, 8.0, 3, 3, 40), (2.0, 3.0, 2, 2, 12), (1.5, 0.0, 5, 1, 30)]
    with api.Context(w, h, 1, 1) as ctx:
        bufs = [_upload([p], [len(p)], dx[None], dy[None], 2048) for _ in pars]
        torch.cuda.synchronize()
        for b, par in zip(bufs, pars):
            _queue(ctx, b, par)
        ctx.sync()
        for k, (b, par) in enumerate(zip(bufs, pars)):
            counts, _ = _check(b, par, what=f"queued call {k}")
            assert counts[0] > 0


def _discs(w, h):
    f = np.full((h, w), 30, np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    for cx, cy, r, v in ((30, 30, 14, 200), (66, 44, 20, 120), (40, 62, 9, 250)):
        f[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = v
    return f


def _state(ctx):
    return (ctx.get_thresholds(), ctx.last_run_info(), ctx.hysteresis_schedule(), ctx.hysteresis_totals(), ctx.hysteresis_info())


@pytest.mark.parametrize("blur", [None, (5, 1.0)], ids=["plain", "blurred"])
def test_canny_circles_equals_the_chain_of_restatements(blur):
    import canny_o_ext_ref as CO
    import deriv_ref as D
    import edge_points_ref as E
    import gauss_blur_ref as G
    w, h = 96, 80
    frames = np.stack([_discs(w, h), _discs(w, h)[::-1].copy()])
    low, high, par = 60, 160, (1.0, 10.0, 12, 5, 30)
    with api.Context(w, h, 1, 2, api.MODE_O) as ctx, api.Context(w, h, 1, 2, api.MODE_O) as other:
        for c in (ctx, other):
            c.set_thresholds(33, 77)
        maps, counts, circles = ctx.canny_circles(frames, low, high, *par, blur=blur)
        plain = other.canny(frames, low, high) if blur is None else other.blur_canny(frames, blur[0], blur[1], low, high)   # the chain without the circles
        assert np.array_equal(maps, plain) and _state(ctx) == _state(other)
        src = frames if blur is None else G.gauss_blur_ref(frames, *blur)
        gx, gy = D.sobel16_frames(src, 3)
        want_maps = np.stack([CO.canny_o(f, low, high, 3, False) for f in src])
        assert np.array_equal(maps, want_maps)
        wc, wcirc = HC.circles_batch([E.points(m) for m in want_maps], gx, gy, w, h, *par)
        assert wc.min() >= 2 and counts.dtype == np.uint32 and counts.tolist() == wc.tolist()
        assert all(a.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(circles, wcirc))
        got = ctx.hough_circles(want_maps, gx, gy, *par, max_circles=2)   # the entry's own convenience, cut lists
        assert got[0].tolist() == wc.tolist() and all(np.array_equal(a.view(np.int32), b[:2].view(np.int32)) for a, b in zip(got[1], wcirc))
    with api.Context(w, h, 3, 1, api.MODE_O) as ctx3, pytest.raises(ValueError, match="1-channel"):
        ctx3.canny_circles(np.zeros((1, h, w, 3), np.uint8), low, high, *par)


def test_refusals_on_a_live_context():
    import torch
    w, h = 33, 31
    p, dx, dy = _scene(w, h, 60)
    par = _params(w, h, 1.0)
    inf, nan = math.inf, math.nan
    with api.Context(w, h, 1, 2) as ctx:
        b = _upload([p, p], [len(p)] * 2, np.stack([dx, dx]), np.stack([dy, dy]), 256)
        torch.cuda.synchronize()
        P, C_, X, Y, O, S = b["d_pts"].data_ptr(), b["d_pc"].data_ptr(), b["d_ax"].data_ptr() + b["off"], b["d_ay"].data_ptr() + b["off"], b["counts"].data_ptr() + 4, b["circles"].data_ptr() + 4 * GUARD
        good = (P, C_, b["pcap"], X, Y, 2 * w, 2 * w * h, 2, *par, 4096, O, S, 256)
        names = ("pts", "pc", "pcap", "dx", "dy", "pitch", "fs", "n", "dp", "min_dist", "thr", "rmin", "rmax", "cc", "counts", "circles", "cap")

        def change(**kw):
            return tuple(kw.get(k, v) for k, v in zip(names, good))
        groups = {
            "null": [change(pts=0), change(pc=0), change(dx=0), change(dy=0), change(counts=0), change(circles=0)],
            "alignment": [change(pts=P + 4), change(pc=C_ + 2), change(counts=O + 1), change(circles=S + 8), change(circles=S + 4, cap=0)],
            "odd views": [change(dx=X + 1), change(dy=Y + 1), change(pitch=2 * w + 1), change(fs=2 * w * h + 1)],
            "view sizes": [change(pitch=2 * w - 2), change(n=1, pitch=((1 << 32) // h + 2) & ~1), change(fs=2 * w * h - 2)],
            "nframes": [change(n=0), change(n=-1), change(n=3)],
            "dp": [change(dp=v) for v in (0.5, 0.0, -1.0, inf, nan, 1e300)],
            "min_dist": [change(min_dist=v) for v in (-1.0, inf, nan)],
            "threshold": [change(thr=-1)],
            "radii": [change(rmin=0), change(rmin=-3), change(rmin=7, rmax=6), change(rmin=1, rmax=4095), change(rmax=(1 << 20) - w), change(rmin=(1 << 20) - h - 10, rmax=(1 << 20) - h)],
            "centre_capacity": [change(cc=0), change(cc=4097)],
            "overflow": [change(pcap=(1 << 64) // 16 + 1), change(cap=(1 << 64) // 32 + 1)],
        }
        for group, calls in groups.items():
            for args in calls:
                with pytest.raises(api.HipCannyError, match="error -1"):
                    ctx.hough_circles_device(*args)
                assert "hc_hough_circles_device" in api.last_error(), group
            ctx.sync()
            torch.cuda.synchronize()
            assert (b["counts"].cpu().numpy() == CANARY).all() and (b["circles"].cpu().numpy() == CANARY).all(), group
            fresh = _upload([p, p[:50]], [len(p), 50], np.stack([dx, dx]), np.stack([dy, dy]), 256)
            torch.cuda.synchronize()
            _queue(ctx, fresh, par)
            ctx.sync()
            counts, _ = _check(fresh, par, what=f"a valid call after the {group} refusals")
            assert counts[0] > 0
        assert api.load_library().hc_hough_circles_device(None, *good) == -1   # ctx null
