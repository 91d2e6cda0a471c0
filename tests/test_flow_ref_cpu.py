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
