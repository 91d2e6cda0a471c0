"""tests/ccl_ref.py, the restatement hc_connected_components_device is tested against, without a GPU: hand-made known answers,
equality with scipy.ndimage.label (where scipy imports) and statistics against sums computed independently with np.bincount."""
import numpy as np
import pytest

import ccl_ref as R


def _one(m, conn):
    labels, counts, stats, cents = R.connected_components(np.asarray(m, np.uint8)[None], conn)
    return labels[0], int(counts[0]), stats[0], cents[0]


def test_u_shape_numbers_do_not_skip():
    """The arms of a U are met before its base: two raster-first candidates merge, and the next component is number 2."""
    m = np.array([[1, 0, 1, 0, 0],
                  [1, 0, 1, 0, 9],
                  [1, 1, 1, 0, 9]])
    for conn in (4, 8):
        lab, n, st, cen = _one(m, conn)
        assert n == 3
        assert lab.tolist() == [[1, 0, 1, 0, 0], [1, 0, 1, 0, 2], [1, 1, 1, 0, 2]]
        assert st.tolist() == [[1, 0, 4, 3, 6], [0, 0, 3, 3, 7], [4, 1, 1, 2, 2]]
        assert cen.tolist() == [[np.float64(15) / np.float64(6), np.float64(4) / np.float64(6)], [1.0, np.float64(8) / np.float64(7)], [4.0, 1.5]]


@pytest.mark.parametrize("w", [1, 5, 9])
def test_diagonal(w):
    m = np.eye(w, dtype=np.uint8) * 255
    lab, n, st, _ = _one(m, 8)
    assert n == 2 and np.array_equal(lab, (m != 0).astype(np.int32))
    if w > 1:
        assert st[1].tolist() == [0, 0, w, w, w]
    lab, n, st, cen = _one(m, 4)
    assert n == w + 1 and np.array_equal(lab, np.diag(np.arange(1, w + 1)).astype(np.int32))
    assert st[1:].tolist() == [[k, k, 1, 1, 1] for k in range(w)] and cen[1:].tolist() == [[float(k), float(k)] for k in range(w)]


@pytest.mark.parametrize("size", [(1, 1), (2, 2), (9, 7), (200, 150)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_checkerboard(size):
    w, h = size
    yy, xx = np.mgrid[0:h, 0:w]
    m = ((xx + yy) % 2 == 0).astype(np.uint8)
    assert _one(m, 8)[1] == 2
    lab, n, st, _ = _one(m, 4)
    assert n == (w * h + 1) // 2 + 1
    assert np.array_equal(lab[m != 0], np.arange(1, n))   # raster order
    assert (st[1:, 4] == 1).all()


@pytest.mark.parametrize("size", [(1, 1), (9, 7), (200, 150)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_isolated_pixels(size):
    w, h = size
    m = np.zeros((h, w), np.uint8)
    m[::2, ::2] = 200
    want = ((w + 1) // 2) * ((h + 1) // 2)
    if size == (200, 150):
        assert want == 7500
    for conn in (4, 8):
        lab, n, st, cen = _one(m, conn)
        assert n == want + 1
        assert np.array_equal(lab[m != 0], np.arange(1, n))
        assert np.array_equal(st[1:, :2], cen[1:].astype(np.int32)) and (st[1:, 2:] == 1).all()


def test_full_empty_and_one_pixel_frames():
    for w, h in ((1, 1), (9, 7)):
        for conn in (4, 8):
            lab, n, st, cen = _one(np.zeros((h, w)), conn)
            assert n == 1 and not lab.any() and st.tolist() == [[0, 0, w, h, w * h]]
            assert cen.tolist() == [[(w - 1) / 2, (h - 1) / 2]]
            lab, n, st, cen = _one(np.full((h, w), 7), conn)
            assert n == 2 and (lab == 1).all()
            assert st.tolist() == [[0, 0, 0, 0, 0], [0, 0, w, h, w * h]]   # the background row of a full frame is all zero
            assert cen.tolist() == [[0.0, 0.0], [(w - 1) / 2, (h - 1) / 2]]


def test_capacity_cuts_the_rows_not_the_labels():
    rng = np.random.default_rng(5)
    maps = (rng.random((2, 20, 30)) < 0.3).astype(np.uint8)
    full = R.connected_components(maps, 8)
    for cap in (0, 1, 3, 10 ** 6):
        labels, counts, stats, cents = R.connected_components(maps, 8, cap)
        assert np.array_equal(labels, full[0]) and np.array_equal(counts, full[1])
        for f in range(2):
            k = min(int(counts[f]), cap)
            assert stats[f].shape == (k, 5) and cents[f].shape == (k, 2)
            assert np.array_equal(stats[f], full[2][f][:k]) and np.array_equal(cents[f], full[3][f][:k])


@pytest.mark.parametrize("conn", [4, 8])
def test_equals_scipy_label(conn):
    ndi = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), int) if conn == 8 else None
    rng = np.random.default_rng(100 + conn)
    for k in range(120):
        h, w = (int(v) for v in rng.integers(1, 41, 2))
        m = (rng.random((h, w)) < rng.choice([0.1, 0.3, 0.5, 0.6, 0.9])).astype(np.uint8) * rng.integers(1, 256, (h, w), dtype=np.uint8)
        lab, n = R.label(m, conn)
        want, k2 = ndi.label(m != 0, structure)
        assert n == k2 + 1 and np.array_equal(lab, want), (k, w, h)


@pytest.mark.parametrize("conn", [4, 8])
def test_stats_against_bincount(conn):
    rng = np.random.default_rng(7 + conn)
    for w, h, dens in ((33, 21, 0.4), (64, 48, 0.55), (130, 67, 0.03)):
        m = (rng.random((h, w)) < dens).astype(np.uint8)
        lab, n = R.label(m, conn)
        ys, xs = np.mgrid[0:h, 0:w]
        flat = lab.reshape(-1)
        area = np.bincount(flat, minlength=n)
        sx = np.bincount(flat, weights=xs.reshape(-1), minlength=n)   # (float64 sums of small integers: exact)
        sy = np.bincount(flat, weights=ys.reshape(-1), minlength=n)
        for st, cen in (R.stats_fast(lab, n), R.stats_of(lab, n)):
            assert np.array_equal(st[:, 4], area)
            assert np.array_equal(cen[:, 0], sx / area) and np.array_equal(cen[:, 1], sy / area)
            for k in range(n):
                sel = np.argwhere(lab == k)
                assert st[k, :4].tolist() == [sel[:, 1].min(), sel[:, 0].min(), np.ptp(sel[:, 1]) + 1, np.ptp(sel[:, 0]) + 1]


@pytest.mark.parametrize("size", [(9, 7), (65, 64), (130, 67)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_closed_forms_equal_the_fill(size):
    """checkerboard4 and columns, the references of the large GPU cases (a fill of 4.4 M pixels is not a test's business), against
    the flood fill at sizes it takes in its stride: labels, N, statistics, and the centroids in their bits."""
    w, h = size
    yy, xx = np.mgrid[0:h, 0:w]

    def same(got, m, conn):
        lab, n, st, cen = _one(m, conn)
        assert got[1] == n and got[0].dtype == np.int32 and np.array_equal(got[0], lab)
        assert got[2].dtype == np.int32 and got[2].shape == (n, 5) and np.array_equal(got[2], st)
        assert got[3].dtype == np.float64 and got[3].shape == (n, 2) and np.array_equal(got[3].view(np.int64), cen.view(np.int64))
    same(R.checkerboard4(w, h), ((xx + yy) % 2 == 0).astype(np.uint8) * 255, 4)
    for x1 in (0, 1, w // 2, w - 1, w):
        for conn in (4, 8):
            same(R.columns(w, h, x1), (xx < x1).astype(np.uint8) * 255, conn)


def test_the_closed_forms_beyond_32_bits():
    """At 2100 x 2100 the sums of x and of y pass 2^32; the centroid of a rectangle is still its middle, exactly."""
    w = h = 2100
    assert w * h * (h - 1) // 2 > 1 << 32
    _, n, st, cen = R.columns(w, h, w)
    assert n == 2 and st.tolist() == [[0, 0, 0, 0, 0], [0, 0, w, h, w * h]] and cen.tolist() == [[0.0, 0.0], [1049.5, 1049.5]]
    _, n, st, cen = R.columns(w, h, 0)
    assert n == 1 and st.tolist() == [[0, 0, w, h, w * h]] and cen.tolist() == [[1049.5, 1049.5]]
    _, n, st, cen = R.columns(w, h, w // 2)
    assert st.tolist() == [[1050, 0, 1050, h, 1050 * h], [0, 0, 1050, h, 1050 * h]] and cen.tolist() == [[1574.5, 1049.5], [524.5, 1049.5]]
