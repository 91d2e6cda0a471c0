"""hc_hough_lines_device (k_hough_vote, k_hough_peaks, k_hough_scan, k_hough_rank) on the MI355X: line counts and lines equal,
value for value, in order and float bits included, to the numpy restatement tests/hough_ref.py.  Every call writes its counts
between two guard words and its lines into a buffer pre-filled with a canary with guard space on both sides -- everything but
the first min(count, line_capacity) lines of each frame's slot must still hold the canary -- and reads a point list that must
come back unchanged; the slots of the list behind a frame's points hold (0, 0), which would vote if a reader strayed there.

The shapes are the smallest at which the paths differ: frames from 1 x 1 to 250 x 200, one angle and angle counts that are no
multiple of the rows per workgroup, point counts around the wave size, cut lists, line capacities around the count, threshold 0
(every local maximum, many ties) and a threshold above every vote, several passes forced by a small scratch bound, one
1920 x 1080 frame (one 24 KB accumulator row per workgroup: a lone frame gets one angle per workgroup) and a batch of nine, by
the plan's rule (two rows) and with six and three rows forced: 144 KB and 72 KB of dynamic LDS, above the 64 KiB a kernel gets
without being told."""
import math

import numpy as np
import pytest

import hough_ref as R
from cudacam_amd import api, synth

pytestmark = pytest.mark.gpu

CANARY = -0x5A5A5A5B
GUARD = 64
PI = math.pi
GEOS = [(1.0, PI / 180, 0.0, PI), (0.5, PI / 90, 0.0, PI), (2.0, PI / 180, 0.0, PI), (3.7, PI / 7, 0.0, PI), (0.3, 0.1, 0.0, PI),
        (1.0, PI / 180, 0.3, 1.2), (1.0, 4.0, 0.0, PI)]   # the last: one angle
SIZES = [(1, 1), (7, 5), (64, 48), (61, 33), (250, 200)]


def _points(w, h, count, seed):
    """`count` points of a w x h frame: two segments and noise, in raster order as k_edge_emit writes them."""
    rng = np.random.default_rng(seed)
    m = np.zeros((h, w), bool)
    t = np.arange(max(w, h) * 2) / 2.0
    for (x0, y0, dx, dy) in ((0, h * 0.3, 1.0, 0.21), (w * 0.6, 0, 0.13, 1.0)):
        x, y = np.rint(x0 + t * dx).astype(int), np.rint(y0 + t * dy).astype(int)
        ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        m[y[ok], x[ok]] = True
    m |= rng.random((h, w)) < 0.05
    pts = R.points_of(m)
    if len(pts) < count:
        pts = R.points_of(np.ones((h, w), bool))
    keep = np.sort(rng.choice(len(pts), size=min(count, len(pts)), replace=False))
    return pts[keep]


def _upload(lists, line_capacity, point_capacity=None):
    """The buffers of one call on the point lists `lists` (int32 (k, 2) per frame): the lists and their counts on the device, the
    counts between two guard words and the line slots between guards, pre-filled with the canary."""
    import torch
    n = len(lists)
    pcap = max(max(len(p) for p in lists), 1) if point_capacity is None else point_capacity
    pts = np.zeros((n, pcap, 2), np.int32)
    for f, p in enumerate(lists):
        pts[f, :min(len(p), pcap)] = p[:pcap]
    pcounts = np.array([len(p) for p in lists], np.uint32)   # the full counts, as hc_edge_points_device reports them above the capacity
    return dict(lists=lists, n=n, pcap=pcap, line_capacity=line_capacity, pts=pts, pcounts=pcounts,
                d_pts=torch.from_numpy(pts).cuda(), d_pc=torch.from_numpy(pcounts.view(np.int32)).cuda(),
                counts=torch.full((n + 2,), CANARY, dtype=torch.int32, device="cuda"),
                lines=torch.full((2 * GUARD + 3 * n * line_capacity,), CANARY, dtype=torch.int32, device="cuda"))


def _queue(ctx, b, geo, threshold, null_lines=False):
    """The call itself, on uploaded buffers (torch's stream has been waited for); nothing is waited for afterwards."""
    rho, theta, lo, hi = geo
    ctx.hough_lines_device(b["d_pts"].data_ptr(), b["d_pc"].data_ptr(), b["pcap"], b["n"], rho, theta, threshold, lo, hi, b["counts"].data_ptr() + 4,
                           None if null_lines else b["lines"].data_ptr() + 4 * GUARD, b["line_capacity"])


def _check(b, w, h, geo, threshold, what=""):
    """What a call left behind (the context has been synchronised), compared with the restatement.  Returns (counts, lines per frame)."""
    lists, n, pcap, line_capacity = b["lists"], b["n"], b["pcap"], b["line_capacity"]
    rho, theta, lo, hi = geo
    assert np.array_equal(b["d_pts"].cpu().numpy(), b["pts"]) and np.array_equal(b["d_pc"].cpu().numpy().view(np.uint32), b["pcounts"]), f"{what}: the point lists were written"
    c = b["counts"].cpu().numpy()
    assert c[0] == CANARY and c[-1] == CANARY, f"{what}: a word beside d_line_counts was written"
    got_counts = c[1:-1].view(np.uint32)
    want_counts, want = R.hough_lines_batch([p[:pcap] for p in lists], w, h, rho, theta, threshold, lo, hi, line_capacity)
    assert got_counts.tolist() == want_counts.tolist(), f"{what}: counts {got_counts.tolist()} != {want_counts.tolist()}"
    l = b["lines"].cpu().numpy()
    assert (l[:GUARD] == CANARY).all() and (l[len(l) - GUARD:] == CANARY).all(), f"{what}: the guard around d_lines was written"
    slots = l[GUARD:len(l) - GUARD].reshape(n, line_capacity, 3)
    for f in range(n):
        k = len(want[f])
        assert k == min(int(want_counts[f]), line_capacity)
        wbits = want[f].view(np.int32)
        if not np.array_equal(slots[f, :k], wbits):
            bad = np.flatnonzero((slots[f, :k] != wbits).any(axis=1))
            raise AssertionError(f"{what}: frame {f}: {len(bad)} of {k} lines differ; first (index, hip, numpy): "
                                 f"{[(int(i), slots[f, i].view(np.float32).tolist(), want[f][i].tolist()) for i in bad[:6]]}")
        assert (slots[f, k:] == CANARY).all(), f"{what}: frame {f}: the slot was written behind its {k} lines"
    return got_counts, want


def _call(ctx, w, h, lists, geo, threshold, line_capacity, point_capacity=None, null_lines=False, what=""):
    """One call on the point lists `lists` (int32 (k, 2) per frame); everything is compared with the restatement.  Returns
    (counts, lines per frame)."""
    import torch
    b = _upload(lists, line_capacity, point_capacity)
    torch.cuda.synchronize()
    _queue(ctx, b, geo, threshold, null_lines)
    ctx.sync()
    return _check(b, w, h, geo, threshold, what)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_size_and_geometry(size):
    w, h = size
    for gi, geo in enumerate(GEOS):
        lists = [_points(w, h, c, 100 * gi + k) for k, c in enumerate((w * h // 6 + 2, 1, min(w * h, 65)))]
        thr = max(2, min(w, h) // 3)
        with api.Context(w, h, 1, 3, api.MODE_O if gi % 2 else api.MODE_R) as ctx:   # either mode
            t = f"{w}x{h} geo {gi}"
            counts, _ = _call(ctx, w, h, lists, geo, thr, 32, what=t)
            _call(ctx, w, h, lists, geo, 0, 64, what=t + " threshold 0")
            _call(ctx, w, h, lists[:1], geo, thr, 0, null_lines=True, what=t + " counts only")


def test_point_counts_around_the_wave_size():
    w, h = 64, 48
    with api.Context(w, h, 1, 3) as ctx:
        for c in (0, 1, 63, 64, 65, 511, 512, 513, 2500):
            lists = [_points(w, h, c, c)]
            assert len(lists[0]) == c
            _call(ctx, w, h, lists, GEOS[0], 0 if c < 66 else 6, 50, what=f"{c} points")
        # three frames with different counts in one call, an empty one among them
        lists = [_points(w, h, 700, 1), np.zeros((0, 2), np.int32), _points(w, h, 65, 2)]
        counts, _ = _call(ctx, w, h, lists, GEOS[0], 5, 40, what="three frames")
        assert counts[1] == 0 and counts[0] > 0


def test_a_list_cut_by_its_capacity_votes_with_what_it_holds():
    w, h = 61, 33
    lists = [_points(w, h, 400, 3), _points(w, h, 90, 4)]
    with api.Context(w, h, 1, 2) as ctx:
        full, _ = _call(ctx, w, h, lists, GEOS[0], 4, 64, what="whole lists")
        cut, _ = _call(ctx, w, h, lists, GEOS[0], 4, 64, point_capacity=100, what="lists cut at 100")   # frame 0 is cut, frame 1 is not
        assert cut[1] == full[1] and cut[0] != full[0]


def test_line_capacities_and_thresholds():
    w, h = 250, 200
    lists = [_points(w, h, 2000, 5), _points(w, h, 1200, 6)]
    with api.Context(w, h, 1, 2) as ctx:
        counts, _ = _call(ctx, w, h, lists, GEOS[0], 20, 0, what="capacity 0, a pointer")
        c0, c1 = int(counts[0]), int(counts[1])
        assert c0 > 2 and c1 > 2 and c0 != c1
        for cap in sorted({1, c0 - 1, c0, c0 + 5, c1 - 1, c1, c1 + 5}):
            _call(ctx, w, h, lists, GEOS[0], 20, cap, what=f"capacity {cap}")
        counts, _ = _call(ctx, w, h, lists, GEOS[0], 0, 100, what="threshold 0")   # every non-empty local maximum: many ties
        assert counts.min() > 1000
        counts, _ = _call(ctx, w, h, lists, GEOS[4], 0, 3000, what="threshold 0, rho 0.3")
        counts, _ = _call(ctx, w, h, lists, GEOS[0], 3001, 10, what="a threshold above every vote")
        assert counts.tolist() == [0, 0]


def test_angle_counts_that_are_no_multiple_of_the_rows_per_workgroup():
    """Batches of 7 x 5 frames that fill the chip, so that a workgroup takes HOUGH_MAX_ROWS = 8 angles: 180 = 22 x 8 + 4 and
    52 = 6 x 8 + 4 at 40 frames, and all 7 angles of theta = pi / 7 in one workgroup at 260 frames."""
    w, h = 7, 5
    lists = [_points(w, h, 3 + k % 9, k) for k in range(260)]
    with api.Context(w, h, 1, 260) as ctx:
        for geo, n in ((GEOS[0], 40), (GEOS[5], 40), (GEOS[3], 260)):
            _call(ctx, w, h, lists[:n], geo, 1, 8, what=f"{n} frames, theta {geo[1]:.4f}")


def test_points_outside_the_frame_vote_where_they_can_and_write_nowhere_else():
    w, h = 64, 48
    big = 1 << 30
    far = np.array([(big, big), (-big, 5), (3, -big), (-big, -big), (big, -big), (-2147483648, 2147483647), (2147483647, 2147483647),
                    (-1, -1), (w, h), (-40, 20), (70, -9), (200, 200), (-300, 7)], np.int32)
    inside = _points(w, h, 300, 9)
    with api.Context(w, h, 1, 2) as ctx:
        for geo in GEOS[:5]:
            _call(ctx, w, h, [np.concatenate([far, inside]), far], geo, 3, 40, what=f"far points, rho {geo[0]}")
            _call(ctx, w, h, [far], geo, 0, 200, what=f"far points alone, rho {geo[0]}")


def test_several_passes_equal_one():
    w, h, n = 64, 48, 5
    lists = [_points(w, h, 200 + 150 * k, 20 + k) for k in range(n)]
    numangle, numrho = R.geometry(w, h, 1.0, PI / 180)
    per_frame = (numangle + 2) * (numrho + 2) * 4 + numangle * ((numrho + 1) // 2) * 8 + numangle * 4
    with api.Context(w, h, 1, n) as ctx:
        one, want = _call(ctx, w, h, lists, GEOS[0], 6, 30, what="one pass")
        for frames in (1, 2, 3, 4):   # 5, 3, 2 and 2 passes
            ctx.set_option(api.OPT_TEST_HOUGH_SCRATCH, frames * per_frame + 17)
            got, _ = _call(ctx, w, h, lists, GEOS[0], 6, 30, what=f"{frames} frames per pass")
            assert got.tolist() == one.tolist()
        ctx.set_option(api.OPT_TEST_HOUGH_SCRATCH, per_frame - 1)
        with pytest.raises(api.HipCannyError, match="error -1"):
            _call(ctx, w, h, lists, GEOS[0], 6, 30, what="a bound below one frame")
        ctx.set_option(api.OPT_TEST_HOUGH_SCRATCH, 0)   # the default again
        _call(ctx, w, h, lists, GEOS[1], 6, 30, what="other tables on the same context")
        _call(ctx, w, h, lists, GEOS[0], 6, 30, what="and back")


def test_scratch_and_tables_replaced_with_calls_in_flight():
    """Four calls on one context with no synchronisation between them: each finds the one before it still queued or running on the
    context stream when it replaces what that call reads -- (b) a larger scratch than (a)'s, (c) other tables in the same
    allocation, (d) more angles than the table allocation holds (and a larger scratch again).  Each writes into buffers of its
    own, which are compared only after the one synchronisation at the end."""
    import torch
    w, h = 64, 48
    lists = [_points(w, h, 300 + 100 * k, 50 + k) for k in range(4)]
    steps = [("a: one frame", lists[:1], (1.0, PI / 180, 0.0, PI)), ("b: four frames, the scratch grows", lists, (1.0, PI / 180, 0.0, PI)),
             ("c: 90 angles, new tables in the old allocation", lists, (1.0, PI / 90, 0.0, PI)), ("d: 360 angles, the tables are reallocated", lists, (1.0, PI / 360, 0.0, PI))]
    assert R.geometry(w, h, 1.0, PI / 90)[0] < R.geometry(w, h, 1.0, PI / 180)[0] < R.geometry(w, h, 1.0, PI / 360)[0]
    bufs = [_upload(ls, 30) for _, ls, _ in steps]
    torch.cuda.synchronize()
    with api.Context(w, h, 1, 4) as ctx:
        for b, (_, _, geo) in zip(bufs, steps):
            _queue(ctx, b, geo, 6)
        ctx.sync()
        for b, (what, _, geo) in zip(bufs, steps):
            counts, _ = _check(b, w, h, geo, 6, what)
            assert counts.min() > 0, what


def test_1080p_three_lines_and_noise():
    w, h = 1920, 1080
    rng = np.random.default_rng(11)
    m = rng.random((h, w)) < 0.01
    t = np.arange(2 * w) / 2.0
    for (x0, y0, dx, dy) in ((0, 200, 1.0, 0.35), (300, 0, 0.4, 1.0), (0, 1000, 1.0, -0.45)):
        x, y = np.rint(x0 + t * dx).astype(int), np.rint(y0 + t * dy).astype(int)
        ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        m[y[ok], x[ok]] = True
    pts = R.points_of(m)
    with api.Context(w, h, 1, 1) as ctx:
        # a drawn line of slope 0.35 - 0.45 spreads over a few bins of one degree: its best cell holds a few hundred of its ~2000 points,
        # far above the ~20000 noise points' cells (26543 points over 6001 bins: about 5 per cell)
        counts, want = _call(ctx, w, h, [pts], GEOS[0], 150, 64, what="1080p")
        assert 3 <= counts[0] <= 64 and want[0][0, 2] > 200


def test_1080p_batch_with_six_rows_in_lds():
    """Nine frames of 1920 x 1080: by the plan's rule (two angles per workgroup, 48 KB), then with HC_OPT_TEST_HOUGH_ROWS 6 --
    k_hough_vote runs with 6 x 6003 x 4 = 144 072 bytes of dynamic LDS, the path on which its launcher raises the kernel's
    bound above 64 KiB --, 3 (72 KB) and 1.  Every run is compared bit for bit with the restatement, and all give the same."""
    w, h, n = 1920, 1080, 9
    t = np.arange(2 * w) / 2.0
    lists = []
    for k in range(n):
        rng = np.random.default_rng(300 + k)
        m = rng.random((h, w)) < 0.004
        for (x0, y0, dx, dy) in ((0, 100 + 90 * k, 1.0, 0.05 * k), (200 + 150 * k, 0, 0.1 * k - 0.3, 1.0)):
            x, y = np.rint(x0 + t * dx).astype(int), np.rint(y0 + t * dy).astype(int)
            ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
            m[y[ok], x[ok]] = True
        lists.append(R.points_of(m))
    with api.Context(w, h, 1, n) as ctx:
        counts, want = _call(ctx, w, h, lists, GEOS[0], 150, 32, what="9 x 1080p")
        assert counts.min() >= 1 and all(l[0, 2] > 150 for l in want)   # a drawn line in every frame, above the noise (11 k points over 6001 bins)
        for rows in (6, 3, 1):
            ctx.set_option(api.OPT_TEST_HOUGH_ROWS, rows)
            again, _ = _call(ctx, w, h, lists, GEOS[0], 150, 32, what=f"9 x 1080p, {rows} rows forced")
            assert again.tolist() == counts.tolist()


@pytest.mark.parametrize("pipelined", [False, True])
def test_hough_lines_and_canny_lines(pipelined):
    w, h, n = 250, 200, 3
    frames = np.stack([synth.natural(w, h, 40 + k) for k in range(n)])
    geo = dict(rho=1.0, theta=PI / 180, threshold=25)
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        if pipelined:
            ctx.set_option(api.OPT_PIPELINE, 1)
        maps = ctx.canny(frames, 50, 150)
        assert maps.any()
        lists = [R.points_of(m) for m in maps]
        want_counts, want = R.hough_lines_batch(lists, w, h, 1.0, PI / 180, 25)
        assert want_counts.min() > 0
        counts, lines = ctx.hough_lines(maps, **geo)   # the counts passes size both buffers
        assert counts.dtype == np.uint32 and counts.tolist() == want_counts.tolist()
        assert all(a.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(lines, want))
        import torch
        counts, lines = ctx.hough_lines(torch.from_numpy(maps).cuda(), max_lines=2, **geo)   # torch maps, cut line lists
        assert counts.tolist() == want_counts.tolist() and all(np.array_equal(a.view(np.int32), b[:2].view(np.int32)) for a, b in zip(lines, want))
        cut_counts, cut = R.hough_lines_batch([p[:300] for p in lists], w, h, 1.0, PI / 180, 25)
        counts, lines = ctx.hough_lines(maps[0], point_capacity=300, **geo)   # one map, a cut point list
        assert counts.tolist() == cut_counts[:1].tolist() and np.array_equal(lines[0].view(np.int32), cut[0].view(np.int32))
        for blur in (None, (5, 1.2)):
            got_maps, counts, lines = ctx.canny_lines(frames, 50, 150, blur=blur, **geo)
            if blur is None:
                assert np.array_equal(got_maps, maps)
            wc, wl = R.hough_lines_batch([R.points_of(m) for m in got_maps], w, h, 1.0, PI / 180, 25)
            assert counts.tolist() == wc.tolist() and len(lines) == n
            assert all(a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(lines, wl))


def test_not_a_run():
    import torch
    w, h, n = 250, 65, 2
    frames = np.stack([synth.natural(w, h, 60 + k) for k in range(n)])
    d_in = torch.from_numpy(frames).cuda()
    d_out = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        maps = ctx.canny(frames, 50, 150)
        before = (ctx.hysteresis_schedule(), ctx.last_run_info(), ctx.pipeline_slots_in_use(), ctx.hysteresis_totals(), ctx.hysteresis_info())
        assert before[0]["launches"] > 0
        lists = [R.points_of(m) for m in maps]
        _call(ctx, w, h, lists, GEOS[0], 10, 16, what="after a run")
        _call(ctx, w, h, lists, GEOS[0], 10, 0, null_lines=True, what="after a run, counts only")
        after = (ctx.hysteresis_schedule(), ctx.last_run_info(), ctx.pipeline_slots_in_use(), ctx.hysteresis_totals(), ctx.hysteresis_info())
        assert before == after
        ctx.set_thresholds(50, 150)
        ctx.run_device(d_in.data_ptr(), w, w * h, d_out.data_ptr(), w, w * h, n)
        ctx.sync()
        info = ctx.last_run_info()
        _call(ctx, w, h, lists, GEOS[0], 10, 16, what="between two runs")
        ctx.run_device(d_in.data_ptr(), w, w * h, d_out.data_ptr(), w, w * h, n)
        ctx.sync()
        assert ctx.last_run_info() == info


def test_argument_errors():
    import torch
    w, h = 16, 8
    pts = torch.zeros((2, 8, 2), dtype=torch.int32, device="cuda")
    pc = torch.full((2,), 8, dtype=torch.int32, device="cuda")
    counts = torch.full((4,), CANARY, dtype=torch.int32, device="cuda")
    lines = torch.full((2 * 8 * 3 + 4,), CANARY, dtype=torch.int32, device="cuda")
    p, q, c, l = pts.data_ptr(), pc.data_ptr(), counts.data_ptr(), lines.data_ptr()
    torch.cuda.synchronize()
    T = PI / 180
    inf, nan = math.inf, math.nan
    with api.Context(w, h, 1, 2) as ctx:
        good = (p, q, 8, 1, 1.0, T, 1, 0.0, PI, c, l, 8)

        def change(**kw):
            names = ("points", "pcounts", "pcap", "n", "rho", "theta", "thr", "lo", "hi", "counts", "lines", "lcap")
            return tuple(kw.get(k, v) for k, v in zip(names, good))
        bad = [change(points=0), change(pcounts=0), change(counts=0), change(lines=0), change(points=p + 4), change(pcounts=q + 2), change(counts=c + 1),
               change(lines=l + 2), change(n=0), change(n=-1), change(n=3), change(thr=-1), change(hi=-0.5), change(lo=1.0, hi=0.5),
               change(rho=1e-4), change(theta=1e-9), change(lcap=(1 << 64) // 12 + 1), change(pcap=(1 << 64) // 8)]
        bad += [change(rho=v) for v in (0.0, -1.0, inf, nan)] + [change(theta=v) for v in (0.0, -1.0, inf, nan)]
        bad += [change(lo=v) for v in (inf, -inf, nan)] + [change(hi=v) for v in (inf, nan)]
        for args in bad:
            with pytest.raises(api.HipCannyError, match="error -1"):
                ctx.hough_lines_device(*args)
        assert api.load_library().hc_hough_lines_device(None, p, q, 8, 1, 1.0, T, 1, 0.0, PI, c, l, 8) == -1   # ctx null
        ctx.sync()
        torch.cuda.synchronize()
        assert (counts.cpu().numpy() == CANARY).all() and (lines.cpu().numpy() == CANARY).all()
        ctx.hough_lines_device(*change(n=2))   # the same buffers are fine for a good call: 8 points at (0, 0)
        ctx.sync()
        assert counts.cpu().numpy()[:2].tolist() == [1, 1]   # rho 0 at the first angle: 8 votes, and right of it an equal cell (a > left fails there)
