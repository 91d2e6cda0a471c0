"""Hand-checked cases of tests/hough_segments_ref.py, the numpy restatement of hc_hough_segments_device: what the GPU tests compare
the kernels with is itself compared with segments worked out by hand."""
import math

import numpy as np

import hough_ref as R
import hough_segments_ref as S

PI = math.pi
W, H = 40, 30
GEO = (1.0, PI / 4, 0.0, PI)   # four angles: 0 (vertical lines), 45 degrees, 90 degrees (horizontal lines), 135 degrees
TT = R.tables(W, H, *GEO)[2]


def _segs(m, lines, min_length, max_gap, capacity=None, geo=GEO, w=W, h=H):
    return S.segments_of(m, np.array(lines, np.float32).reshape(-1, 3), w, h, *geo, min_length, max_gap, capacity)


def test_walk_tables_of_four_angles():
    major, slope, scale = S.walk_tables(W, H, *GEO)
    # theta 0: x = rho, one sample per row; float32(pi / 4) lies above pi / 4: |sin| >= |cos|, one sample per column; three times
    # that float lies above 3 pi / 4: |sin| < |cos|, one sample per row again
    assert major.tolist() == [1, 0, 0, 1]
    assert slope[0] == 0 and scale[0] == 1           # x = rho
    assert abs(slope[1] + 1) < 1e-6 and abs(scale[1] - math.sqrt(2)) < 1e-6      # y = -x + rho * sqrt(2)
    assert abs(slope[2]) < 1e-6 and abs(scale[2] - 1) < 1e-6                     # y = rho
    assert abs(slope[3] - 1) < 1e-6 and abs(scale[3] + math.sqrt(2)) < 1e-6      # x = y - rho * sqrt(2)
    assert (np.abs(S.walk_tables(250, 200, 0.3, 0.01, -1.0, 2.5)[1]) <= 1).all()


def test_horizontal_vertical_and_diagonal_lines_come_back_whole():
    m = np.zeros((H, W), np.uint8)
    m[7, 5:31] = 255                       # horizontal: y = 7, theta 90 degrees, rho 7
    m[3:22, 11] = 255                      # vertical: x = 11, theta 0, rho 11
    count, segs = _segs(m, [(7, TT[2], 0), (11, TT[0], 0)], 5, 0)
    assert count == 2 and segs.tolist() == [[5, 7, 30, 7], [11, 3, 11, 21]]
    d = np.zeros((H, W), np.uint8)
    assert S.draw(d, W, H, *GEO, 3, -5.0, 10, 25) == 16   # 135 degrees, a step per row: x = y + 7.07 -> rint: (17, 10) .. (32, 25)
    count, segs = _segs(d, [(-5.0, TT[3], 0)], 5, 0)
    assert count == 1 and segs.tolist() == [[17, 10, 32, 25]]
    assert d.sum() == 16 * 255 and all(d[y, x] for x, y in zip(range(17, 33), range(10, 26)))
    e = np.zeros((H, W), np.uint8)
    assert S.draw(e, W, H, *GEO, 1, 20.0, 5, 20) == 16    # 45 degrees, a step per column: y = -x + 28.28 -> rint: (5, 23) .. (20, 8)
    assert _segs(e, [(20.0, TT[1], 0)], 5, 0)[1].tolist() == [[5, 23, 20, 8]] and all(e[y, x] for x, y in zip(range(5, 21), range(23, 7, -1)))


def test_a_gap_of_max_gap_joins_and_one_more_splits():
    m = np.zeros((H, W), np.uint8)
    m[7, 2:10] = 255
    m[7, 13:20] = 255                      # columns 10, 11, 12 are missing: a gap of 3
    line = [(7, TT[2], 0)]
    assert _segs(m, line, 0, 3)[1].tolist() == [[2, 7, 19, 7]]
    assert _segs(m, line, 0, 2)[1].tolist() == [[2, 7, 9, 7], [13, 7, 19, 7]]
    assert _segs(m, line, 0, 0)[0] == 2
    assert S.groups_of([1, 2, 4, 9, 10], 1) == [(1, 4), (9, 10)] and S.groups_of([], 3) == [] and S.groups_of([5], 0) == [(5, 5)]


def test_a_length_of_exactly_min_length_is_kept_and_a_unit_less_is_dropped():
    m = np.zeros((H, W), np.uint8)
    m[7, 2:8] = 255                        # (2, 7) .. (7, 7): squared length 25
    line = [(7, TT[2], 0)]
    assert _segs(m, line, 5, 0)[0] == 1 and _segs(m, line, 6, 0)[0] == 0
    d = np.zeros((H, W), np.uint8)
    S.draw(d, W, H, *GEO, 3, -5.0, 10, 13)    # (17, 10) .. (20, 13): squared length 18: kept at 4 (16), dropped at 5 (25)
    assert _segs(d, [(-5.0, TT[3], 0)], 4, 0)[1].tolist() == [[17, 10, 20, 13]] and _segs(d, [(-5.0, TT[3], 0)], 5, 0)[0] == 0


def test_single_pixels_are_kept_only_at_min_length_zero():
    m = np.zeros((H, W), np.uint8)
    m[7, 4] = m[7, 20] = 255
    line = [(7, TT[2], 0)]
    assert _segs(m, line, 0, 3)[1].tolist() == [[4, 7, 4, 7], [20, 7, 20, 7]]
    assert _segs(m, line, 1, 3)[0] == 0


def test_lines_that_address_nothing():
    m = np.full((H, W), 255, np.uint8)
    for line in [(H + 50, TT[2], 0), (-1, TT[2], 0), (1e30, TT[0], 0), (math.nan, TT[2], 0), (math.inf, TT[2], 0), (-math.inf, TT[1], 0),
                 (7, np.float32(1.0), 0), (7, np.float32(math.nan), 0), (7, np.nextafter(TT[2], np.float32(9)), 0)]:
        assert _segs(m, [line], 0, 0)[0] == 0, line
    assert _segs(m, [(7, TT[2], 0)], 0, 0)[1].tolist() == [[0, 7, W - 1, 7]]      # the same map, a line inside it
    assert _segs(m, [(H - 1, TT[2], 0), (H, TT[2], 0)], 0, 0)[0] == 1             # the last row, and the row behind it


def test_end_points_ascend_with_the_step_and_lines_keep_their_order():
    m = np.zeros((H, W), np.uint8)
    S.draw(m, W, H, *GEO, 1, 20.0, 0, W - 1)   # 45 degrees: y = -x + 28.28: y falls as the step (x) rises
    m[12, :] = 255
    count, segs = _segs(m, [(12, TT[2], 0), (20.0, TT[1], 0)], 3, 0)
    assert count == 2 and segs[0].tolist() == [0, 12, W - 1, 12]
    x0, y0, x1, y1 = segs[1].tolist()
    assert x0 < x1 and y0 > y1 and (x0, y0) == (0, 28)
    assert _segs(m, [(20.0, TT[1], 0), (12, TT[2], 0)], 3, 0)[1][1].tolist() == [0, 12, W - 1, 12]   # the other order of lines
    m[12, 10:13] = 0
    assert _segs(m, [(12, TT[2], 0)], 3, 0)[1].tolist() == [[0, 12, 9, 12], [13, 12, W - 1, 12]]     # along the line: ascending


def test_cut_by_capacity_the_count_stays_full():
    m = np.zeros((H, W), np.uint8)
    m[7, ::2] = 255
    full = _segs(m, [(7, TT[2], 0)], 0, 0)
    assert full[0] == 20 and len(full[1]) == 20
    cut = _segs(m, [(7, TT[2], 0)], 0, 0, capacity=3)
    assert cut[0] == 20 and cut[1].tolist() == full[1][:3].tolist() and cut[1].dtype == np.int32
    none = _segs(m, [(7, TT[2], 0)], 0, 0, capacity=0)
    assert none[0] == 20 and none[1].shape == (0, 4)
    counts, segs = S.segments_batch([m, m * 0], [np.array([(7, TT[2], 0)], np.float32)] * 2, W, H, *GEO, 0, 0, 5)
    assert counts.dtype == np.uint32 and counts.tolist() == [20, 0] and len(segs[0]) == 5 and len(segs[1]) == 0
