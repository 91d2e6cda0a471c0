"""tests/flow_ref.py, the numpy restatement of hc_pyr_down_device and hc_lk_flow_device, against direct restatements and against
flows that are known by construction.  No GPU."""
import numpy as np
import pytest

import flow_ref as R


def pyr_down_loops(src):
    """the header's formula, one destination pixel at a time"""
    h, w = src.shape
    t = [1, 4, 6, 4, 1]
    out = np.zeros(((h + 1) // 2, (w + 1) // 2), np.uint8)
    for y in range(out.shape[0]):
        for x in range(out.shape[1]):
            s = 0
            for j in range(-2, 3):
                for i in range(-2, 3):
                    s += t[i + 2] * t[j + 2] * int(src[R.reflect101(2 * y + j, h), R.reflect101(2 * x + i, w)])
            out[y, x] = (s + 128) >> 8
    return out


@pytest.mark.parametrize("w,h", [(3, 3), (4, 5), (37, 23)])
def test_pyr_down_matches_the_double_loop(w, h):
    src = np.random.default_rng(w * 100 + h).integers(0, 256, (h, w), dtype=np.uint8)
    got = R.pyr_down(src)
    assert got.shape == ((h + 1) // 2, (w + 1) // 2)
    assert np.array_equal(got, pyr_down_loops(src))


@pytest.mark.parametrize("value", [0, 1, 127, 255])
def test_pyr_down_keeps_a_constant_image(value):
    assert np.all(R.pyr_down(np.full((11, 14), value, np.uint8)) == value)


def test_reflect101():
    assert [R.reflect101(i, 5) for i in (-2, -1, 0, 4, 5, 6)] == [2, 1, 0, 4, 3, 2]


def smooth(w, h, sx, sy):
    """a sum of a few low-frequency sinusoids, sampled at (x + sx, y + sy)"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = x + sx, y + sy
    v = (128 + 40 * np.sin(x * 0.11 + 0.3) * np.cos(y * 0.13) + 30 * np.sin(x * 0.05 + y * 0.09 + 1.0) + 25 * np.cos(x * 0.17 - y * 0.07)
         + 20 * np.sin(y * 0.21 + 0.5))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def grid_points():
    gx, gy = np.meshgrid(np.linspace(16, 79, 7), np.linspace(16, 63, 7))
    return np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float32)[None]


def shifted_pair(sx, sy):
    """next(x, y) = prev(x - sx, y - sy): what is at p in prev is at p + (sx, sy) in next"""
    return smooth(96, 80, 0, 0)[None], smooth(96, 80, -sx, -sy)[None]


def test_small_shift_is_recovered_at_one_level():
    """Bound 0.053 px: the reference's largest position error on this pair is 0.0264 px (the u8 quantisation of both frames and the
    bilinear model of a curved surface), doubled for the choice of content."""
    prev, nxt = shifted_pair(1.3, -0.7)
    pts = grid_points()
    got, status, err = R.optical_flow(prev, nxt, pts, [49], win=21, levels=0)
    assert np.all(status == 1)
    worst = np.abs(got[0] - pts[0] - np.float32([1.3, -0.7])).max()
    print("largest position error", worst)
    assert worst <= 0.053
    assert np.all(err >= 0) and err.max() < 2


def test_large_shift_is_recovered_with_three_levels():
    """Bound 0.039 px: the reference's largest position error on this pair is 0.0192 px, doubled for the choice of content."""
    prev, nxt = shifted_pair(5.2, 3.6)
    pts = grid_points()
    got, status, _ = R.optical_flow(prev, nxt, pts, [49], win=21, levels=3)
    assert np.all(status == 1)
    worst = np.abs(got[0] - pts[0] - np.float32([5.2, 3.6])).max()
    print("largest position error", worst)
    assert worst <= 0.039


def test_pyramid_stops_at_sides_of_three():
    assert [p.shape for p in R.pyramid(np.zeros((9, 40), np.uint8), 5)] == [(9, 40), (5, 20), (3, 10)]
    assert len(R.pyramid(np.zeros((5, 5), np.uint8), 3)) == 2
    assert len(R.pyramid(np.zeros((4, 40), np.uint8), 3)) == 1


def test_flat_patch_is_lost_and_left_unchanged():
    prev, nxt = np.full((1, 40, 48), 90, np.uint8), np.full((1, 40, 48), 90, np.uint8)
    pts = np.float32([[[20.25, 18.5]]])
    got, status, err = R.lk_level(prev, nxt, 0, [1], pts, np.zeros_like(pts), 7, 10, 0.01, 1e-4, 0, np.full((1, 1), 9, np.uint8), np.full((1, 1), 9, np.float32))
    assert status[0, 0] == 0 and err[0, 0] == 0
    assert np.array_equal(got, pts)


def test_far_outside_is_lost_and_left_unchanged():
    prev, nxt = shifted_pair(1.0, 0.0)
    for pt in ([-500.0, 10.0], [10.0, 1e12], [np.nan, 5.0]):
        pts = np.float32([[pt]])
        got, status, _ = R.lk_level(prev, nxt, 0, [1], pts, np.zeros_like(pts), 9, 10, 0.01, 1e-4, 0, np.full((1, 1), 9, np.uint8))
        assert status[0, 0] == 0
        assert np.array_equal(got.view(np.uint32), pts.view(np.uint32))


def test_lost_with_a_guess_keeps_the_guess():
    prev, nxt = np.full((1, 40, 48), 7, np.uint8), np.full((1, 40, 48), 7, np.uint8)
    pts, guess = np.float32([[[20, 20]]]), np.float32([[[23.5, 19.25]]])
    got, status, _ = R.lk_level(prev, nxt, 0, [1], pts, guess, 7, 10, 0.01, 1e-4, 1, np.zeros((1, 1), np.uint8))
    assert status[0, 0] == 0 and np.array_equal(got, guess)


def test_the_guess_is_the_start():
    """A shift beyond one level's reach from the point itself is found from a guess next to it; one iteration moves from the guess."""
    prev, nxt = shifted_pair(9.0, -6.0)
    pts = np.float32([[[40, 40]]])
    guess = pts + np.float32([8.5, -5.5])
    got, status, _ = R.lk_level(prev, nxt, 0, [1], pts, guess, 21, 30, 0.01, 1e-4, 1, np.zeros((1, 1), np.uint8))
    assert status[0, 0] == 1
    assert np.abs(got[0, 0] - pts[0, 0] - np.float32([9.0, -6.0])).max() < 0.1
    one, _, _ = R.lk_level(prev, nxt, 0, [1], pts, guess, 21, 1, 0.0, 1e-4, 1, np.zeros((1, 1), np.uint8))
    assert np.abs(one[0, 0] - guess[0, 0]).max() < 1.0 and not np.array_equal(one, guess)


def test_levels_above_zero_leave_status_and_err():
    prev, nxt = shifted_pair(2.0, 2.0)
    p1, n1 = R.pyr_down(prev[0])[None], R.pyr_down(nxt[0])[None]
    pts = np.float32([[[40, 40]]])
    got, status, err = R.lk_level(p1, n1, 1, [1], pts, np.zeros_like(pts), 11, 30, 0.01, 1e-4, 0, np.full((1, 1), 7, np.uint8), np.full((1, 1), 5, np.float32))
    assert status[0, 0] == 7 and err[0, 0] == 5
    assert np.abs(got[0, 0] - pts[0, 0] - np.float32([2.0, 2.0])).max() < 0.2


def test_slots_beyond_the_count_are_untouched():
    prev, nxt = shifted_pair(1.0, 1.0)
    pts = np.float32([[[40, 40], [30, 30], [50, 20]]])
    start = np.full_like(pts, -3)
    got, status, _ = R.lk_level(prev, nxt, 0, [2], pts, start, 9, 10, 0.01, 1e-4, 0, np.full((1, 3), 9, np.uint8))
    assert np.array_equal(got[0, 2], start[0, 2]) and status[0, 2] == 9 and np.all(status[0, :2] == 1)


# ---- what the cases of tests/test_gpu_flow.py are for, by the reference alone (tests/flow_cases.py) --------------------------
import flow_cases as FC  # noqa: E402


def test_info_reports_the_exact_sums():
    """A11, A12, A22, B1 / B2 per iteration and err_sum are the integers the float steps start from: restated here from the
    reference's own template and compared, at a tracked point and a lost one."""
    a, b = FC.pair(48, 40, 0)
    pt = np.float32([20.25, 17.5])
    out, st, err, info = R.lk_point(a, b, 0, pt, pt, 7, 30, 0.01, 1e-4, 0)
    assert st == 1 and info["lost"] is None and len(info["B1"]) == len(info["B2"]) == info["iterations"] >= 2
    jj, ii = np.mgrid[0:7, 0:7]
    ix, iy, wts = R._weights((np.float32(pt[0] - 3), np.float32(pt[1] - 3)))
    gx = (R._interp(lambda x, y: R._scharr(a, x, y)[0], ix, iy, wts, ii, jj) + 8192) >> 14
    gy = (R._interp(lambda x, y: R._scharr(a, x, y)[1], ix, iy, wts, ii, jj) + 8192) >> 14
    I = (R._interp(lambda x, y: R._pix(a, x, y), ix, iy, wts, ii, jj) + 256) >> 9
    J = (R._interp(lambda x, y: R._pix(b, x, y), ix, iy, wts, ii, jj) + 256) >> 9
    assert (info["A11"], info["A12"], info["A22"]) == (int((gx * gx).sum()), int((gx * gy).sum()), int((gy * gy).sum()))
    assert (info["B1"][0], info["B2"][0]) == (int(((J - I) * gx).sum()), int(((J - I) * gy).sum()))
    assert err == np.float32(np.float32(info["err_sum"]) / np.float32(32 * 49))
    flat = R.lk_point(np.full((40, 48), 9, np.uint8), b, 0, pt, pt, 7, 30, 0.01, 1e-4, 0)
    assert flat[1] == 0 and flat[3]["lost"] == "eigen" and flat[3]["A11"] == flat[3]["A22"] == 0 and flat[3]["B1"] == [] and "err_sum" not in flat[3]
    assert R.lk_point(a, b, 0, np.float32([-50, 3]), pt, 7, 30, 0.01, 1e-4, 0)[3]["lost"] == "start"


def test_the_windows_cover_every_kernel_and_every_idle_round():
    """flow_rounds / flow_round_class (canny_params.h) restated: the windows of the device test reach each of the six compiled
    kernels, and in each kernel that can have wholly idle rounds a window that has them."""
    assert FC.WINDOWS == tuple(w for w in range(5, 32) if w & 1) and len(FC.WINDOWS) == 14
    assert [FC.flow_rounds(w) for w in FC.WINDOWS] == [1, 1, 2, 2, 3, 4, 5, 6, 7, 9, 10, 12, 14, 16]
    assert {FC.flow_round_class(w) for w in FC.WINDOWS} == set(FC.ROUND_CLASSES)
    assert {w: FC.idle_rounds(w) for w in FC.WINDOWS if FC.idle_rounds(w)} == {13: 1, 17: 2, 19: 1, 23: 1, 27: 4, 29: 2}
    assert {FC.flow_round_class(w) for w in FC.WINDOWS if FC.idle_rounds(w)} == {4, 7, 10, 16}
    assert all(w * w % 64 for w in FC.WINDOWS)   # and every window's last round is partly filled: the `t < ww` guards


@pytest.mark.parametrize("win", FC.WINDOWS)
def test_every_window_has_tracked_lost_and_iterating_points(win):
    a, b, pts, starts = FC.window_case(win)
    assert a.shape == (FC.WIN_H, FC.WIN_W)
    left = 0
    for (iters, eps, init, _), start in zip(FC.WIN_RUNS, starts):
        inf = FC.infos(a, b, 0, pts, start, win, iters, eps, 1e-4, init)
        lost = [i["lost"] for _, i in inf]
        assert all((st == 1) == (why is None) for (st, _), why in zip(inf, lost))
        assert lost.count(None) >= 1, "no point is tracked"
        assert lost.count("eigen") >= 1, "no point is lost by the eigenvalue rule"
        assert sum(why in ("start", "left", "end") for why in lost) >= 1, "no point is lost by leaving the frame"
        assert sum(i["iterations"] >= 2 for _, i in inf) >= 1, "no point takes two iterations"
        left += lost.count("left")
    if win != 27:   # (at 27 every point that starts inside stays inside, in all four runs)
        assert left >= 1, "no point leaves the frame while it iterates"


def test_every_kernel_has_a_point_that_leaves_while_it_iterates():
    seen = set()
    for win in FC.WINDOWS:
        a, b, pts, starts = FC.window_case(win)
        if any(i["lost"] == "left" for _, i in FC.infos(a, b, 0, pts, starts[0], win, *FC.WIN_RUNS[0][:2], 1e-4, 0)):
            seen.add(FC.flow_round_class(win))
    assert seen == set(FC.ROUND_CLASSES)


@pytest.mark.parametrize("win", FC.TINY_WINDOWS)
@pytest.mark.parametrize("w,h", FC.TINY_SHAPES)
def test_planes_smaller_than_the_window(w, h, win):
    """1 x 1, 1 x 9 and 9 x 1 have no gradient in one direction at least: every point is lost, by the eigenvalue rule or by its
    position.  6 x 5 has tracked points at both windows."""
    a, b, pts = FC.tiny_case(w, h, win)
    assert a.shape == (h, w)
    for init in (0, 1):
        inf = FC.infos(a, b, 0, pts, pts + np.float32(0.5), win, 30, 0.01, 1e-4, init)
        lost = [i["lost"] for _, i in inf]
        assert "eigen" in lost or (w, h) == (6, 5)
        assert "start" in lost
        if (w, h) == (6, 5):
            assert lost.count(None) >= 3 and max(i["iterations"] for _, i in inf) >= 2
        else:
            assert set(lost) == {"eigen", "start"}


def test_level_15_has_tracked_and_lost_points():
    a, b, pts, start = FC.top_level_case()
    assert a.shape == (FC.TOP_H, FC.TOP_W) and FC.TOP_LEVEL == 15
    for init in (0, 1):
        inf = FC.infos(a, b, FC.TOP_LEVEL, pts, start, FC.TOP_WIN, 30, 0.01, 1e-4, init)
        lost = [i["lost"] for _, i in inf]
        assert all(st is None for st, _ in inf)
        assert lost.count(None) >= 3 and "start" in lost and "left" in lost
        got = R.lk_level(a[None], b[None], FC.TOP_LEVEL, [len(pts)], pts[None], start[None], FC.TOP_WIN, 30, 0.01, 1e-4, init)[0][0]
        moved = [k for k, why in enumerate(lost) if why is None]
        # next is prev rolled by one column: in level-0 units a tracked point moves by about 32768 in x
        assert np.median(got[moved, 0] - pts[moved, 0]) > 16384 and not np.array_equal(got[moved], (start if init else pts)[moved])


def test_some_points_run_all_64_iterations():
    a, b, pts = FC.long_case()
    inf = FC.infos(a, b, 0, pts, pts, FC.LONG_WIN, 64, 0.0, 1e-4, 0)
    full = [k for k, (st, i) in enumerate(inf) if i["iterations"] == 64 and i["lost"] is None]
    assert len(full) >= 3 and all(len(inf[k][1]["B1"]) == 64 for k in full)
    assert any(2 <= i["iterations"] < 64 for _, i in inf)
    at = lambda k, iters: R.lk_point(a, b, 0, pts[k], pts[k], FC.LONG_WIN, iters, 0.0, 1e-4, 0)[0]
    assert any(not np.array_equal(at(k, 64), at(k, 63)) for k in full)   # the 64th iteration moves them


def test_window_sums_leave_32_bits():
    """The blocks: sums of squares at or above 2^32 and sums of difference times gradient at or beyond +-2^31, at points that are
    tracked -- so the high dwords of the device's 64-bit wave sums decide next_pts."""
    a11 = a22 = low = high = 0
    for roll in FC.BIG_ROLLS:
        a, b, pts = FC.big_sum_case(roll)
        assert a.shape == (FC.BIG_H, FC.BIG_W) and set(np.unique(a)) == {0, 255}
        for win in FC.BIG_WINDOWS:
            for st, i in FC.infos(a, b, 0, pts, pts, win, 30, 0.01, 1e-4, 0):
                bs = i["B1"] + i["B2"]
                beyond = i["A11"] >= 2 ** 32 or i["A22"] >= 2 ** 32 or min(bs) <= -2 ** 31 or max(bs) >= 2 ** 31
                if not beyond:
                    continue
                assert st == 1, "a point with a sum beyond 32 bits is lost"
                a11 += i["A11"] >= 2 ** 32
                a22 += i["A22"] >= 2 ** 32
                low += min(bs) <= -2 ** 31
                high += max(bs) >= 2 ** 31
    print("points with A11 >= 2^32:", a11, "A22 >= 2^32:", a22, "a B <= -2^31:", low, "a B >= 2^31:", high)
    assert a11 >= 1 and a22 >= 1 and low >= 1 and high >= 1


def test_sixteen_lane_sums_leave_32_bits():
    """The stripes: a sum at or beyond +-2^33 is four sixteen-lane sums of which one at least is at or beyond +-2^31."""
    a11 = low = high = 0
    for roll in FC.STRIPE_ROLLS:
        a, b, pts = FC.stripe_sum_case(roll)
        for win in FC.STRIPE_WINDOWS:
            for st, i in FC.infos(a, b, 0, pts, pts, win, 30, 0.01, 1e-4, 0):
                assert st == 1 and i["iterations"] >= 2
                a11 += i["A11"] >= 2 ** 33
                low += min(i["B1"]) <= -2 ** 33
                high += max(i["B1"]) >= 2 ** 33
    assert a11 >= 2 and low >= 1 and high >= 1


def test_eight_lane_sums_leave_32_bits():
    """The horizontal stripes at window 31: with lane t % 64 owning window pixel t = j * 31 + i (flow.hip), a sum of diff * gy over
    eight consecutive lanes is beyond -2^31 (rolled down) and 2^31 (rolled up) in the first iteration, no sum over four lanes is
    (it cannot be: 4 x 16 x 8160 x 4080 < 2^31), and the points are tracked."""
    low = high = 0
    for roll in FC.ROW_ROLLS:
        a, b, pts = FC.row_sum_case(roll)
        for (st, i), pt in zip(FC.infos(a, b, 0, pts, pts, FC.ROW_WIN, 30, 0.01, 1e-4, 0), pts):
            px, py = FC.first_products(a, b, pt, FC.ROW_WIN)
            assert (int(px.sum()), int(py.sum())) == (i["B1"][0], i["B2"][0])
            assert st == 1 and i["iterations"] >= 2
            assert max(abs(v) for v in FC.lane_group_sums(py, 4)) < 2 ** 31
            low += min(FC.lane_group_sums(py, 8)) <= -2 ** 31
            high += max(FC.lane_group_sums(py, 8)) >= 2 ** 31
    assert low >= 2 and high >= 2


def test_the_early_stop_pyramid_has_three_planes():
    a, b, pts, counts = FC.stop_case()
    assert [p.shape for p in R.pyramid(a[0], FC.STOP_LEVELS)] == [(9, 20), (5, 10), (3, 5)]
    want = R.optical_flow(a, b, pts, counts, win=FC.STOP_WIN, levels=FC.STOP_LEVELS)
    assert want[1][0].sum() >= 3 and want[1][1, :7].sum() >= 3 and not want[1][1, 7:].any()
    two = R.optical_flow(a, b, pts, counts, win=FC.STOP_WIN, levels=2)
    assert all(np.array_equal(x, y) for x, y in zip(want, two))   # levels beyond the stop change nothing
