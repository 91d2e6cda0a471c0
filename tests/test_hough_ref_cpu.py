"""tests/hough_ref.py (the numpy restatement of hc_hough_lines_device) against cases worked out by hand from the contract in
include/hipcanny.h.  No GPU, no OpenCV.

The hand-worked frames are 7 x 5 at rho 1, theta pi / 4 over [0, pi]: four angles (0, 45, 90 and 135 degrees), numrho = 25,
(numrho - 1) / 2 = 12.  With c = 0.7071: a point (x, y) votes at r = x, rint((x + y) c), y and rint((y - x) c)."""
import math

import numpy as np
import pytest

import hough_ref as R

Q = math.pi / 4
F = np.float32
T = [F(0.0), F(Q), F(F(Q) + F(Q)), F(F(F(Q) + F(Q)) + F(Q))]   # the running float angle


def _lines(points, threshold, **kw):
    return R.hough_lines(np.array(points, np.int32), 7, 5, 1.0, Q, threshold, **kw)


def test_geometry_known_answers():
    assert R.geometry(1920, 1080, 1, math.pi / 180, 0, math.pi) == (180, 6001)
    assert R.geometry(64, 48, 1, math.pi / 180, 0.3, 1.2) == (52, 225)
    assert R.geometry(64, 48, 1, math.pi / 4, 0, math.pi) == (4, 225)
    assert R.geometry(64, 48, 1, 4.0, 0, math.pi) == (1, 225)
    assert R.geometry(7, 5, 1, Q) == (4, 25)
    assert R.geometry(64, 48, 2, math.pi / 180)[1] == 112      # 112.5: half to even
    assert R.geometry(65, 48, 2, math.pi / 180)[1] == 114      # 113.5
    assert R.geometry(64, 48, 0.5, math.pi / 90) == (90, 450)


def test_tables_by_hand():
    tc, ts, tt = R.tables(7, 5, 1.0, Q)
    assert tt.tolist() == [float(v) for v in T] and tt.dtype == np.float32
    assert tc[0] == 1.0 and ts[0] == 0.0
    assert tc[1] == F(math.cos(float(F(Q)))) and ts[1] == F(math.sin(float(F(Q))))
    assert abs(float(tc[2])) < 1e-7 and ts[2] == 1.0          # cos of the float nearest pi / 2 is not 0
    assert tc[3] < 0 < ts[3]
    tc2, ts2, _ = R.tables(7, 5, 0.5, Q)                       # irho = 2 scales both
    assert tc2[0] == 2.0 and ts2[2] == 2.0
    _, _, tt3 = R.tables(64, 48, 1.0, math.pi / 180, 0.3, 1.2)
    assert tt3[0] == F(0.3) and tt3[1] == F(F(0.3) + F(math.pi / 180)) and len(tt3) == 52


def test_one_point():
    count, lines = _lines([(3, 2)], 0)
    # r = 3, rint(3.54) = 4, 2, rint(-0.71) = -1: one vote each, all four peaks, tied: ascending accumulator index = ascending n
    assert count == 4
    assert lines.dtype == np.float32 and lines.tolist() == [[3.0, float(T[0]), 1.0], [4.0, float(T[1]), 1.0], [2.0, float(T[2]), 1.0], [-1.0, float(T[3]), 1.0]]
    assert _lines([(3, 2)], 1)[0] == 0                         # a > threshold, not >=
    count, lines = _lines([(3, 2)], 0, capacity=2)
    assert count == 4 and lines.tolist() == [[3.0, 0.0, 1.0], [4.0, float(T[1]), 1.0]]
    assert _lines([], 0)[0] == 0 and _lines([], 0)[1].shape == (0, 3)


def test_horizontal_vertical_and_diagonal_segments():
    hor = [(x, 2) for x in range(7)]
    acc = R.accumulate(np.array(hor, np.int32), 4, 25, *R.tables(7, 5, 1.0, Q)[:2])
    assert acc.shape == (6, 27) and acc.sum() == 7 * 4
    assert acc[3, 2 + 12 + 1] == 7                             # 90 degrees: every point at r = y = 2
    assert acc[1, 13:20].tolist() == [1] * 7                   # 0 degrees: r = x
    assert acc[2, 12 + 1 + 4] == 2 and acc[4, 12 + 1 - 1] == 2 and acc[4, 12 + 1 + 1] == 2   # 45: 3.54 and 4.24 -> 4; 135: two at 1, two at -1
    count, lines = _lines(hor, 2)
    assert count == 1 and lines.tolist() == [[2.0, float(T[2]), 7.0]]
    ver = [(3, y) for y in range(5)]
    count, lines = _lines(ver, 2)
    assert count == 1 and lines.tolist() == [[3.0, 0.0, 5.0]]
    dia = [(k, 4 - k) for k in range(5)]                       # x + y = 4: rint(4 c) = rint(2.83) = 3 at 45 degrees
    count, lines = _lines(dia, 1)
    assert count == 1 and lines.tolist() == [[3.0, float(T[1]), 5.0]]
    # the three together, (3, 2) and (2, 2) now counted more than once: y = 2 holds 7 + 1 + 1 points, x = 3 holds 5 + 1 + 1, and
    # x + y = 4 holds 5 + 1 + 1 as well -- but that cell (45 degrees, r = 3) lies right below (0 degrees, r = 3), which has 7 too:
    # a > up fails, and it is no line
    count, lines = _lines(hor + ver + dia, 5)
    assert count == 2 and lines.tolist() == [[2.0, float(T[2]), 9.0], [3.0, 0.0, 7.0]]


def _acc(numangle, numrho, cells):
    a = np.zeros((numangle + 2, numrho + 2), np.int32)
    for (n, r), v in cells.items():
        a[n + 1, r + 1] = v
    return a


def test_plateaus_show_the_asymmetry_in_both_axes():
    # two equal cells side by side: the LEFT one is the peak (a > left, a >= right)
    v, n, r = R.peaks(_acc(3, 4, {(1, 1): 5, (1, 2): 5}), 3, 4, 0)
    assert (v.tolist(), n.tolist(), r.tolist()) == ([5], [1], [1])
    # two equal cells one above the other: the UPPER one (a > up, a >= down)
    v, n, r = R.peaks(_acc(3, 4, {(0, 2): 4, (1, 2): 4}), 3, 4, 0)
    assert (v.tolist(), n.tolist(), r.tolist()) == ([4], [0], [2])
    # a 2 x 2 plateau: its upper left corner alone
    v, n, r = R.peaks(_acc(3, 4, {(1, 1): 3, (1, 2): 3, (2, 1): 3, (2, 2): 3}), 3, 4, 0)
    assert (v.tolist(), n.tolist(), r.tolist()) == ([3], [1], [1])
    # a strictly larger neighbour on any side kills the cell
    for nb in ((0, 1), (2, 1), (1, 0), (1, 2)):
        v, n, r = R.peaks(_acc(3, 4, {(1, 1): 3, nb: 4}), 3, 4, 0)
        assert (n.tolist(), r.tolist()) == ([nb[0]], [nb[1]])


def test_peaks_in_the_border_rows_and_columns_and_ties_by_index():
    cells = {(0, 0): 2, (0, 3): 2, (2, 0): 2, (2, 3): 2, (1, 2): 2, (0, 2): 1}
    v, n, r = R.peaks(_acc(3, 4, cells), 3, 4, 1)
    # all five 2s are peaks (the padding is 0); tied, so by index (n + 1) * 6 + r + 1
    assert v.tolist() == [2] * 5 and list(zip(n.tolist(), r.tolist())) == [(0, 0), (0, 3), (1, 2), (2, 0), (2, 3)]
    cells[(2, 3)] = 9
    v, n, r = R.peaks(_acc(3, 4, cells), 3, 4, 1)
    assert v.tolist() == [9, 2, 2, 2, 2] and (n[0], r[0]) == (2, 3)
    # votes in the padding columns take part as neighbours but are no lines
    a = _acc(3, 4, {(1, 0): 3, (1, 3): 3})
    a[2, 0] = 3       # left padding of row n = 1: equal, and a > left fails
    a[2, 5] = 4       # right padding: larger, and a >= right fails
    assert len(R.peaks(a, 3, 4, 0)[0]) == 0


@pytest.mark.parametrize("rho", [0.3, 0.5, 1.0, 2.0, 3.7])
def test_no_vote_of_a_point_inside_the_frame_is_dropped(rho):
    for w, h in ((7, 5), (1920, 1080)):
        pts = np.array([(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, h // 3)], np.int32)
        numangle, numrho = R.geometry(w, h, rho, math.pi / 180)
        tc, ts, _ = R.tables(w, h, rho, math.pi / 180)
        acc = R.accumulate(pts, numangle, numrho, tc, ts)
        assert acc.sum() == len(pts) * numangle and acc[0].sum() == 0 and acc[-1].sum() == 0


def test_far_points_vote_nowhere_and_break_nothing():
    big = 1 << 30
    pts = np.array([(big, big), (-big, 5), (3, -big), (-1, -1), (7, 5), (2, 2), (-2147483648, 2147483647)], np.int32)
    numangle, numrho = R.geometry(7, 5, 1.0, Q)
    tc, ts, _ = R.tables(7, 5, 1.0, Q)
    acc = R.accumulate(pts, numangle, numrho, tc, ts)
    near = R.accumulate(pts[3:6], numangle, numrho, tc, ts)   # (-1, -1), (7, 5) and (2, 2) lie within reach of the accumulator
    assert near.sum() == 12
    assert acc.sum() >= 12 and (acc - near).min() >= 0 and (acc - near).sum() <= 4 * 4


def test_accumulate_equals_a_scalar_walk():
    rng = np.random.default_rng(5)
    for w, h, rho, theta in ((61, 33, 3.7, math.pi / 7), (64, 48, 0.5, math.pi / 90), (250, 200, 0.3, 0.1)):
        pts = np.stack([rng.integers(-3, w + 3, 300), rng.integers(-3, h + 3, 300)], axis=1).astype(np.int32)
        numangle, numrho = R.geometry(w, h, rho, theta)
        tc, ts, _ = R.tables(w, h, rho, theta)
        want = np.zeros((numangle + 2, numrho + 2), np.int32)
        for x, y in pts:
            for n in range(numangle):
                s = F(F(F(x) * tc[n]) + F(F(y) * ts[n]))
                r = int(np.rint(s)) + int((numrho - 1) / 2)
                if -1 <= r <= numrho:
                    want[n + 1, r + 1] += 1
        assert np.array_equal(R.accumulate(pts, numangle, numrho, tc, ts), want)
