"""Known answers of the numpy restatement tests/hough_circles_ref.py, worked by hand from the contract in include/hipcanny.h: the
restatement is what the GPU tests compare the device with, so it is pinned here against numbers that do not come from it."""
import numpy as np
import pytest

import hough_circles_ref as HC


def _planes(w, h, at, g):
    dx, dy = np.zeros((h, w), np.int16), np.zeros((h, w), np.int16)
    dx[at[1], at[0]], dy[at[1], at[0]] = g
    return dx, dy


def test_one_point_with_gradient_3_4_both_rays_cell_by_cell():
    """(x, y) = (10, 10), gradient (3, 4), dp 1: mag = 5, x0 = y0 = 10240, sx = rint(3072 / 5) = rint(614.4) = 614, sy = rint(4096 /
    5) = rint(819.2) = 819.  Forward from r = 2: (11468, 11878) -> cell (11, 11); (12082, 12697) -> (11, 12); (12696, 13516) -> (12,
    13); (13310, 14335) -> (12, 13) again.  Backward: (9012, 8602) -> (8, 8); (8398, 7783) -> (8, 7); (7784, 6964) -> (7, 6); (7170,
    6145) -> (7, 6) again: arithmetic shifts of positive numbers."""
    w, h = 20, 16
    dx, dy = _planes(w, h, (10, 10), (3, 4))
    x0, y0, sx, sy = HC.rays([10], [10], [3], [4], 1.0)
    assert (x0[0], y0[0], sx[0], sy[0]) == (10240, 10240, 614, 819)
    acc = HC.accumulate([(10, 10)], dx, dy, w, h, 1.0, 2, 5)
    want = np.zeros((h + 2, w + 2), np.int32)
    for cx, cy, v in ((11, 11, 1), (11, 12, 1), (12, 13, 2), (8, 8, 1), (8, 7, 1), (7, 6, 2)):
        want[cy + 1, cx + 1] = v
    assert np.array_equal(acc, want)


def test_a_ray_is_cut_at_the_border_and_the_other_goes_on():
    """(2, 1), gradient (3, 4), radii 1 .. 6 on 8 x 6.  Backward: r = 1 (2048 - 614, 1024 - 819) = (1434, 205) -> (1, 0); r = 2 (820,
    -614) -> y2 = -1: cut, whatever the later radii would give.  Forward: (2662, 1843) -> (2, 1); (3276, 2662) -> (3, 2); (3890, 3481)
    -> (3, 3); (4504, 4300) -> (4, 4); (5118, 5119) -> (4, 4); (5732, 5938) -> (5, 5): the last row."""
    w, h = 8, 6
    dx, dy = _planes(w, h, (2, 1), (3, 4))
    stats = {}
    acc = HC.accumulate([(2, 1)], dx, dy, w, h, 1.0, 1, 6, stats)
    want = np.zeros((h + 2, w + 2), np.int32)
    for cx, cy, v in ((1, 0, 1), (2, 1, 1), (3, 2, 1), (3, 3, 1), (4, 4, 2), (5, 5, 1)):
        want[cy + 1, cx + 1] = v
    assert np.array_equal(acc, want) and stats["cut_rays"] == 1
    assert HC.accumulate([(2, 1)], dx, dy, w, h, 1.0, 1, 7, {}).sum() == 7   # r = 7: (6346, 6757) -> y2 = 6 is outside: cut as well


def test_negative_fixed_point_shifts_are_arithmetic():
    """(0, 0), gradient (-1, 0): sx = -1024.  Backward (d = -1) walks to the right: x1 = 1024, 2048, ...; forward starts at -1024 >> 10
    = -1: cut at once.  With gradient (1, 1): mag = sqrt(2) rounded, sx = rint(1024 / 1.41421354) = 724; forward r = 1: 724 >> 10 = 0;
    backward: -724 >> 10 = -1 (an arithmetic shift, not a division): cut."""
    w, h = 5, 4
    dx, dy = _planes(w, h, (0, 0), (-1, 0))
    acc = HC.accumulate([(0, 0)], dx, dy, w, h, 1.0, 1, 3)
    assert acc[1, 1:].tolist() == [0, 1, 1, 1, 0, 0] and acc.sum() == 3
    dx, dy = _planes(w, h, (0, 0), (1, 1))
    assert HC.rays([0], [0], [1], [1], 1.0)[2][0] == 724
    acc = HC.accumulate([(0, 0)], dx, dy, w, h, 1.0, 1, 2)
    assert acc[1, 1] == 1 and acc[2, 2] == 1 and acc.sum() == 2   # r = 1: (724, 724) -> (0, 0); r = 2: (1448, 1448) -> (1, 1)


def test_half_to_even_of_x0_and_sx():
    """dp = 2048: idp = 2^-11 and idp * 1024 = 1 / 2, all exact.  x0 = rint(x / 2): x = 1, 3, 5, 7 give 0.5, 1.5, 2.5, 3.5 -> 0, 2, 2, 4.
    sx with vy = 0 (mag = |vx|): rint(+-0.5) = 0 for every vx.  dp = 2048 / 5: idp * 1024 = 2.5 exactly, gradient (0, 5): sy =
    rint(2.5) = 2.  dp = 512: idp * 1024 = 2, gradients (3, 4) and (4, 3): 6 / 5 = 1.2 -> 1 and 8 / 5 = 1.6 -> 2, no half involved."""
    assert HC.rays([1, 3, 5, 7], [0, 0, 0, 0], [1, 1, 1, 1], [0, 0, 0, 0], 2048.0)[0].tolist() == [0, 2, 2, 4]
    assert HC.rays([0, 0, 0], [0, 0, 0], [1, 7, -9], [0, 0, 0], 2048.0)[2].tolist() == [0, 0, 0]
    assert HC.rays([0], [0], [0], [5], 2048.0 / 5)[3][0] == 2
    assert HC.rays([0], [0], [0], [-5], 2048.0 / 5)[3][0] == -2
    r = HC.rays([0, 0], [0, 0], [3, 4], [4, 3], 512.0)
    assert r[2].tolist() == [1, 2] and r[3].tolist() == [2, 1]


def test_the_gradient_minus_32768_twice():
    """m = 2 * 2^30 = 2^31 does not fit int32 but is exact in uint32; (float)m = 2^31, mag = sqrt(2^31) = 46340.95 rounded to float32;
    sx = sy = rint(-32768 * 1024 / mag) = rint(-724.077) = -724."""
    x0, y0, sx, sy = HC.rays([5], [5], [-32768], [-32768], 1.0)
    assert (sx[0], sy[0]) == (-724, -724)
    x0, y0, sx, sy = HC.rays([5], [5], [32767], [-32768], 1.0)
    assert (sx[0], sy[0]) == (724, -724)
    assert HC.rays([5], [5], [-32768], [0], 1.0)[2][0] == -1024 and HC.rays([5], [5], [32767], [0], 1.0)[2][0] == 1024


def test_the_peak_rule_at_the_padding_and_a_tie_by_index():
    """A 3 x 2 accumulator (padded 5 x 4).  Equal neighbours: the left one of a horizontal pair and the upper one of a vertical pair
    win (> towards up and left, >= towards down and right); the padding's zeros are neighbours like any other cell."""
    acc = np.zeros((4, 5), np.int32)
    acc[1, 1:4] = (5, 5, 2)   # row cy = 0: cells cx = 0, 1, 2
    acc[2, 1:4] = (1, 5, 2)   # row cy = 1
    c = HC.centres(acc, 1)
    # (0, 0): 5 > up 0, >= down 1, > left 0, >= right 5: a centre.  (1, 0): left is 5, not smaller: none.  (1, 1): up is 5: none.
    # (2, 0): 2 > 1, left 5: none.  (2, 1): up 2, not smaller: none.  (0, 1): 1 is not above the threshold.
    assert c.tolist() == [[5, 0, 0]]
    acc[2, 2] = 6             # now (1, 1) beats its upper neighbour, and (1, 0) has a larger one below
    assert HC.centres(acc, 1).tolist() == [[6, 1, 1], [5, 0, 0]]
    tie = np.zeros((5, 7), np.int32)
    tie[3, 1], tie[1, 5], tie[1, 2] = 4, 4, 4   # three centres of 4 votes: index order is (2, 0), (5, 0), then (0, 2)
    assert HC.centres(tie, 3).tolist() == [[4, 1, 0], [4, 4, 0], [4, 0, 2]]
    assert HC.centres(tie, 4).tolist() == []    # a centre has MORE votes than the threshold


@pytest.mark.parametrize("md, want", [(0.0, 0), (1.0, 1), (2.5, 7)])
def test_min_d2(md, want):
    """md^2 = 0, 1, 6.25: the smallest integers not below are 0, 1 and 7."""
    assert HC.geometry(64, 48, 2.0, md * 2.0, 1, 10)[2] == want
    assert HC.geometry(64, 48, 1.0, md, 1, 10)[2] == want


def test_geometry_by_hand():
    assert HC.geometry(64, 48, 1.0, 0, 1, 10)[:2] == (64, 48)
    assert HC.geometry(65, 31, 2.0, 0, 1, 10)[:2] == (33, 16)      # 32.5 and 15.5 rounded up
    assert HC.geometry(9, 7, 1.5, 0, 1, 4)[:2] == (6, 5)            # idp = fl(2 / 3) = 0.66666669 in float32: 9 * idp = 6.0000002 rounds to 6.0f -> 6; 4.6666 -> 5
    for bad in ((0, 5, 1.0, 0, 1, 2), (5, 5, 0.99, 0, 1, 2), (5, 5, float("nan"), 0, 1, 2), (5, 5, 1.0, -1, 1, 2), (5, 5, 1.0, float("inf"), 1, 2), (5, 5, 1.0, 0, 0, 2),
                (5, 5, 1.0, 0, 3, 2), (5, 5, 1.0, 0, 1, 4095), (5, 5, 1.0, 0, (1 << 20) - 8, (1 << 20) - 5), (5, 5, 1e300, 0, 1, 2)):
        with pytest.raises(ValueError):
            HC.geometry(*bad)


def test_sift_in_order_with_the_distance_of_the_kept_ones_only():
    ranked = [(9, 10, 10), (8, 12, 10), (7, 14, 10), (7, 10, 13), (6, 30, 30)]
    # min_d2 = 9: (12, 10) is 2 from the first: dropped; (14, 10) is 4 from the first -- and 2 from the DROPPED one, which does not
    # count: kept; (10, 13): 3 from the first, 9 >= 9: kept
    stats = {}
    assert HC.sift(ranked, 9, stats=stats).tolist() == [[9, 10, 10], [7, 14, 10], [7, 10, 13], [6, 30, 30]]
    assert stats == {"dropped": 1, "ties": 1}
    assert HC.sift(ranked, 10).tolist() == [[9, 10, 10], [7, 14, 10], [6, 30, 30]]
    assert HC.sift(ranked, 0).tolist() == [list(r) for r in ranked]
    assert HC.sift(ranked, 9, centre_capacity=2).tolist() == [[9, 10, 10]]   # only the first two go on
    assert HC.sift([], 9).shape == (0, 3)


def test_a_centre_with_two_concentric_radii_and_both_ends_of_the_histogram():
    """Centre cell (10, 10) at dp 1: (fx, fy) = (10.5, 10.5).  (13, 14): ddx = -2.5, ddy = -3.5, rad = sqrt(18.5) = 4.30 -> bin
    rint(4.30 - 2) = 2; four such points by the symmetry x -> 21 - x, y -> 21 - y.  (10, 2): ddx = 0.5, ddy = 8.5, rad = sqrt(72.5) = 8.51
    -> bin rint(6.51) = 7; four such points.  min_radius 2, max_radius 9: hist has 10 words; bins 2 and 7 hold 4."""
    pts = [(13, 14), (8, 14), (13, 7), (8, 7), (10, 2), (11, 19), (2, 10), (19, 11)]
    fx, fy, hist = HC.histogram(pts, 24, 24, 10, 10, 1.0, 2, 9)
    assert (fx, fy) == (10.5, 10.5)
    assert hist.tolist() == [0, 0, 0, 4, 0, 0, 0, 0, 4, 0]   # hist[i + 1] counts radius 2 + i: i = 2 and i = 7
    c = HC.radii(pts, 24, 24, 10, 10, 1.0, 4, 2, 9)
    assert c.tolist() == [[10.5, 10.5, 4.0, 4.0], [10.5, 10.5, 9.0, 4.0]]
    assert HC.radii(pts, 24, 24, 10, 10, 1.0, 5, 2, 9).shape == (0, 4)   # h >= votes_threshold
    # both ends: rad == min_radius and rad == max_radius exactly.  Centre (3, 0) at dp 2: (fx, fy) = (7, 1); (7, 4) is 3 away, (7, 9) is
    # 8 away, (7, 10) is 9 away: outside 3 .. 8; (7, 3) is 2 away: outside
    pts = [(7, 4), (7, 9), (7, 10), (7, 3), (4, 1), (-1, 1), (7, -2)]   # (4, 1): 3 away; (-1, 1) and (7, -2) lie outside the frame
    fx, fy, hist = HC.histogram(pts, 12, 12, 3, 0, 2.0, 3, 8)
    assert (fx, fy) == (7.0, 1.0) and hist.tolist() == [0, 2, 0, 0, 0, 0, 1, 0]
    assert HC.radii(pts, 12, 12, 3, 0, 2.0, 1, 3, 8)[:, 2:].tolist() == [[3.0, 2.0], [8.0, 1.0]]
    # a plateau: equal neighbours -- the smaller radius wins (h > hist[i], h >= hist[i + 2])
    pts = [(7, 4), (7, 5)]
    assert HC.radii(pts, 12, 12, 3, 0, 2.0, 1, 3, 8)[:, 2:].tolist() == [[3.0, 1.0]]


def test_circles_of_a_drawn_scene_end_to_end():
    """Two concentric circles drawn with radial gradients: the strongest centre is theirs and carries both radii."""
    w, h = 64, 48
    dx, dy = np.zeros((h, w), np.int16), np.zeros((h, w), np.int16)
    pts = np.concatenate([HC.draw(dx, dy, w, h, 30, 24, 8), HC.draw(dx, dy, w, h, 30, 24, 15)])
    stats = {}
    count, c = HC.circles_of(pts, dx, dy, w, h, 1.0, 8.0, 20, 4, 20, stats=stats)
    assert count >= 2 and c.dtype == np.float32 and stats["two_radii"] >= 1
    assert abs(c[0, 0] - 30.5) <= 1 and abs(c[0, 1] - 24.5) <= 1 and c[0, 2] == 8 and c[1, 2] == 15 and (c[1, :2] == c[0, :2]).all()
    assert HC.circles_of(pts, dx, dy, w, h, 1.0, 8.0, 20, 4, 20, capacity=1)[1].shape == (1, 4)
    counts, per = HC.circles_batch([pts, pts[:0]], [dx, dx], [dy, dy], w, h, 1.0, 8.0, 20, 4, 20)
    assert counts.dtype == np.uint32 and counts.tolist() == [count, 0] and per[1].shape == (0, 4)
