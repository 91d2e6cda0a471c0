"""tests/deriv_ref.py against independent restatements (no GPU): the aperture 3 / 5 Sobel of canny_o_ext_ref (itself
anchored to the oracle), a float32 emulation of OpenCV's separable float filter for the scaled 7x7 Sobel, direct 2-D
correlations, and known answers."""
import numpy as np
import pytest

import canny_o_ext_ref as X
import deriv_ref as D


def _images():
    rng = np.random.default_rng(7)
    rnd = rng.integers(0, 256, (61, 67), dtype=np.uint8)
    k = np.ones(5) / 5.0
    sm = rng.integers(0, 256, (61, 67)).astype(np.float64)
    for ax in (0, 1):
        sm = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), ax, sm)
    smooth = np.clip(np.rint(sm), 0, 255).astype(np.uint8)
    cb = ((np.add.outer(np.arange(61), np.arange(67)) & 1) * 255).astype(np.uint8)
    col = rng.integers(0, 256, (23, 19, 3), dtype=np.uint8)
    return {"random": rnd, "smooth": smooth, "checker": cb, "zeros": np.zeros((9, 11), np.uint8), "ff": np.full((9, 11), 255, np.uint8),
            "colour": col, "1x1": np.array([[77]], np.uint8), "2x3": rng.integers(0, 256, (3, 2), dtype=np.uint8)}


IMAGES = _images()


def _corr2d(a, kern):
    """Direct 2-D correlation, BORDER_REPLICATE, int64; a is (H,W) or (H,W,C)."""
    a = np.asarray(a).astype(np.int64)
    kern = np.asarray(kern, np.int64)
    r = kern.shape[0] // 2
    h, w = a.shape[:2]
    out = np.zeros(a.shape, np.int64)
    for i in range(kern.shape[0]):
        rows = np.clip(np.arange(h) + i - r, 0, h - 1)
        for j in range(kern.shape[1]):
            cols = np.clip(np.arange(w) + j - r, 0, w - 1)
            out += kern[i, j] * a[rows][:, cols]
    return out


def _float_sep(a, kx, ky):
    """OpenCV's separable filter in float32: the row filter (u8 -> float) with kx, then the column filter with ky, each a
    running float32 sum in tap order; the caller rounds."""
    a = np.asarray(a).astype(np.float32)
    h, w = a.shape[:2]
    r = len(kx) // 2
    row = np.zeros(a.shape, np.float32)
    for j, t in enumerate(kx):
        cols = np.clip(np.arange(w) + j - r, 0, w - 1)
        row = (row + np.float32(t) * a[:, cols]).astype(np.float32)
    out = np.zeros(a.shape, np.float32)
    for i, t in enumerate(ky):
        rows = np.clip(np.arange(h) + i - r, 0, h - 1)
        out = (out + np.float32(t) * row[rows]).astype(np.float32)
    return out


@pytest.mark.parametrize("name", sorted(IMAGES))
@pytest.mark.parametrize("ksize", [3, 5])
def test_3_and_5_equal_sobel_o(name, ksize):
    img = IMAGES[name]
    dx, dy = D.sobel16(img, ksize)
    wx, wy = X.sobel_o(img, ksize)
    assert dx.dtype == np.int16 and dy.dtype == np.int16 and dx.shape == img.shape
    np.testing.assert_array_equal(dx, wx)
    np.testing.assert_array_equal(dy, wy)


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_7_equals_float_emulation_and_2d(name):
    img = IMAGES[name]
    dx, dy = D.sobel16(img, 7)
    s = np.array(D.SMOOTH[7], np.float32) * np.float32(1.0 / 16.0)   # Sobel scales the smoothing kernel
    d = np.array(D.DERIV[7], np.float32)
    fx, fy = _float_sep(img, d, s), _float_sep(img, s, d)
    np.testing.assert_array_equal(dx, np.rint(fx).astype(np.int64))   # cvRound: half to even
    np.testing.assert_array_equal(dy, np.rint(fy).astype(np.int64))
    k2 = np.outer(D.SMOOTH[7], D.DERIV[7])   # rows: smoothing along y, columns: derivative along x
    np.testing.assert_array_equal(dx, D.round_half_even_shift(_corr2d(img, k2), 4))
    np.testing.assert_array_equal(dy, D.round_half_even_shift(_corr2d(img, k2.T), 4))


def test_7_ties_are_common_and_naive_rounding_differs():
    """The tests can tell half-to-even from (S + 8) >> 4: a fair share of pixels are exact ties."""
    for name in ("random", "smooth"):
        sx, sy = D.sums(IMAGES[name], 7)
        s = np.concatenate([sx.ravel(), sy.ravel()])
        ties = (s & 15) == 8
        assert ties.mean() > 0.03
        naive = (s + 8) >> 4
        assert (naive != D.round_half_even_shift(s, 4)).mean() > 0.01
        # the formula the header states
        np.testing.assert_array_equal((s + 7 + ((s >> 4) & 1)) >> 4, D.round_half_even_shift(s, 4))


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_scharr_equals_2d(name):
    img = IMAGES[name]
    dx, dy = D.sobel16(img, -1)
    k2 = np.array([[-3, 0, 3], [-10, 0, 10], [-3, 0, 3]])
    np.testing.assert_array_equal(dx, _corr2d(img, k2))
    np.testing.assert_array_equal(dy, _corr2d(img, k2.T))


def _step():
    a = np.zeros((15, 16), np.uint8)
    a[:, 8:] = 255
    return a


def _ramp():
    return np.tile(np.arange(32, dtype=np.uint8), (15, 1))


def test_known_answers_7():
    dx, dy = D.sobel16(_step(), 7)
    assert (np.abs(dx[:, 7]) == 10200).all() and (np.abs(dx[:, 8]) == 10200).all() and (dx[:, 7] > 0).all()
    assert (dy == 0).all()
    dx, dy = D.sobel16(_ramp(), 7)
    assert (dx[:, 3:-3] == 128).all() and (dy == 0).all()
    r, c = 7, 7
    a = np.zeros((15, 15), np.uint8)
    a[r, c] = 8
    dx, _ = D.sobel16(a, 7)
    assert dx[r + 3, c - 1] == 2      # 2.5 -> 2
    assert dx[r + 3, c + 1] == -2     # -2.5 -> -2
    assert dx[r + 1, c - 1] == 38     # 37.5 -> 38
    assert dx[r + 3, c + 3] == 0      # -0.5 -> 0


def test_known_answers_scharr():
    dx, dy = D.sobel16(_step(), -1)
    assert (dx[:, 7] == 4080).all() and (dx[:, 8] == 4080).all() and (dy == 0).all()
    dx, dy = D.sobel16(_ramp(), -1)
    assert (dx[:, 1:-1] == 32).all() and (dy == 0).all()


def test_ranges():
    cb = IMAGES["checker"]
    for ksize, bound in ((3, 1020), (5, 12240), (7, 10200), (-1, 4080)):
        for img in (cb, _step(), _step().T.copy()):
            dx, dy = D.sobel16(img, ksize)
            assert max(np.abs(dx).max(), np.abs(dy).max()) <= bound
        dx, dy = D.sobel16(_step(), ksize)
        assert np.abs(dx).max() == bound
