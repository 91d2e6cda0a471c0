"""tests/gauss_blur_ref.py anchored without a GPU: the properties the stated arithmetic must have (constants, the impulse
response, one-pixel shifts under both borders), a brute-force double loop on frames smaller than the radius, the taps rule,
and the C function hc_gaussian_taps_q8 against the Python one through ctypes (the library loads without a GPU).  No OpenCV
is installed: nothing here is pinned against a build of it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cudacam_amd import api, build
import gauss_blur_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMAS = (0.5, 0.8, 1.0, 1.4, 2.0, 5.0)
TAP_SETS = ([G.gaussian_taps_q8(k, s) for k in G.KSIZES for s in (0.0,) + SIGMAS]
            + [[256, 0, 0], [0, 0, 256], [0, 0, 0, 0, 256], [256, 0, 0, 0, 0, 0, 0], [1, 200, 55], [3, 0, 100, 120, 33], [7, 9, 0, 40, 150, 0, 50]])


def border_index(i, n, border):
    """cv::borderInterpolate, written out."""
    if border == G.REPLICATE:
        return min(max(i, 0), n - 1)
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * (n - 1) - i
    return i


def brute(img, taps, border):
    h, w = img.shape[:2]
    a = img.reshape(h, w, -1).astype(int)
    r = len(taps) // 2
    out = np.zeros(a.shape, np.uint8)
    for ch in range(a.shape[2]):
        for y in range(h):
            for x in range(w):
                v = 0
                for j, tj in enumerate(taps):
                    yy = border_index(y + j - r, h, border)
                    hs = sum(ti * a[yy, border_index(x + i - r, w, border), ch] for i, ti in enumerate(taps))
                    assert hs <= 65280
                    v += tj * hs
                out[y, x, ch] = (v + 32768) >> 16
    return out.reshape(img.shape)


@pytest.mark.parametrize("value", [0, 1, 127, 255])
def test_constant_frames_come_back(value):
    for taps in TAP_SETS:
        for border in G.BORDERS:
            for shape in ((6, 9), (2, 3, 3), (1, 1)):
                img = np.full(shape, value, np.uint8)
                assert np.array_equal(G.blur(img, taps, border), img), (taps, border, shape)


def test_impulse_response_is_the_mirrored_outer_product():
    for taps in TAP_SETS:
        k = len(taps)
        r = k // 2
        img = np.zeros((15, 17), np.uint8)
        img[7, 8] = 255
        out = G.blur(img, taps).astype(int)
        want = np.zeros_like(out)
        for j in range(k):       # a correlation: the output at (7 + r - j, 8 + r - i) sees the impulse under taps (j, i)
            for i in range(k):
                want[7 + r - j, 8 + r - i] = (255 * taps[i] * taps[j] + 32768) >> 16
        assert np.array_equal(out, want), taps


@pytest.mark.parametrize("border", G.BORDERS)
def test_one_tap_shifts_the_image(border):
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (7, 9), dtype=np.uint8)
    # [256, 0, 0]: every output pixel is its neighbour up-left (tap 0 multiplies the pixel one column / row before)
    out = G.blur(img, [256, 0, 0], border)
    assert np.array_equal(out[1:, 1:], img[:-1, :-1])
    edge = 1 if border == G.REFLECT_101 else 0   # what index -1 maps to
    assert np.array_equal(out[1:, 0], img[:-1, edge]) and np.array_equal(out[0, 1:], img[edge, :-1]) and out[0, 0] == img[edge, edge]
    out = G.blur(img, [0, 0, 256], border)
    assert np.array_equal(out[:-1, :-1], img[1:, 1:])
    ey, ex = (5, 7) if border == G.REFLECT_101 else (6, 8)   # what indices 7 (rows) and 9 (columns) map to
    assert np.array_equal(out[:-1, -1], img[1:, ex]) and np.array_equal(out[-1, :-1], img[ey, 1:]) and out[-1, -1] == img[ey, ex]


@pytest.mark.parametrize("border", G.BORDERS)
@pytest.mark.parametrize("k", G.KSIZES)
def test_brute_force_on_frames_below_the_radius(k, border):
    rng = np.random.default_rng(100 * k + border)
    sets = [G.gaussian_taps_q8(k, 0.0), G.gaussian_taps_q8(k, 1.4), [t for t in TAP_SETS if len(t) == k][-1]]
    for w, h in ((1, 1), (2, 3), (3, 1), (5, 2), (9, 8)):
        for ch in (1, 3):
            img = rng.integers(0, 256, (h, w) if ch == 1 else (h, w, ch), dtype=np.uint8)
            for taps in sets:
                assert np.array_equal(G.blur(img, taps, border), brute(img, taps, border)), (w, h, ch, taps)


def test_fixed_tables_at_sigma_zero():
    assert G.gaussian_taps_q8(3, 0) == [64, 128, 64]
    assert G.gaussian_taps_q8(5, 0) == [16, 64, 96, 64, 16]
    assert G.gaussian_taps_q8(7, 0.0) == [8, 28, 56, 72, 56, 28, 8]
    assert G.gaussian_taps_q8(5, -1.0) == [16, 64, 96, 64, 16]
    for k in G.KSIZES:
        assert api.gaussian_taps_q8(k, 0) == G.gaussian_taps_q8(k, 0)


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("k", G.KSIZES)
def test_taps_from_sigma(k, sigma):
    t = G.gaussian_taps_q8(k, sigma)
    assert len(t) == k and t == t[::-1] and sum(t) == 256 and min(t) >= 0 and max(t) <= 256
    assert all(t[i] <= t[i + 1] for i in range(k // 2)), t   # a non-increasing tail on either side of the centre
    assert api.gaussian_taps_q8(k, sigma) == t
    G.check_taps(t)


def test_wide_and_narrow_sigmas_keep_the_contract():
    for k in G.KSIZES:
        for sigma in (1e-300, 1e-160, 1e-3, 0.05, 0.3, 10.0, 1e3, 1e300):
            t = G.gaussian_taps_q8(k, sigma)
            assert sum(t) == 256 and t == t[::-1] and 0 <= min(t) and max(t) <= 256, (k, sigma, t)
            assert api.gaussian_taps_q8(k, sigma) == t


@pytest.fixture(scope="module")
def lib():
    build.build()
    return api.load_library()


def test_c_function_equals_the_python_one(lib):
    rng = np.random.default_rng(7)
    sigmas = [0.0, -2.0, 1e-300, 1e-160, 1e-3, 0.05, 1e3, 1e300] + list(SIGMAS) + [float(s) for s in rng.uniform(0.05, 6.0, 300)]
    for k in G.KSIZES:
        for sigma in sigmas:
            buf = (C.c_uint16 * 8)(*([0xABCD] * 8))
            assert lib.hc_gaussian_taps_q8(k, sigma, buf) == 0, api.last_error()
            assert list(buf[:k]) == api.gaussian_taps_q8(k, sigma) == G.gaussian_taps_q8(k, sigma), (k, sigma)
            assert list(buf[k:]) == [0xABCD] * (8 - k)


def test_c_function_refusals(lib):
    buf = (C.c_uint16 * 8)(*([0xABCD] * 8))
    for k, sigma in ((4, 1.0), (1, 1.0), (9, 1.0), (0, 0.0), (-1, 0.0), (3, float("nan")), (5, float("inf")), (7, float("-inf"))):
        assert lib.hc_gaussian_taps_q8(k, sigma, buf) == -1 and "hc_gaussian_taps_q8" in api.last_error(), (k, sigma)
        assert list(buf) == [0xABCD] * 8
    assert lib.hc_gaussian_taps_q8(3, 1.0, None) == -1
    for k, sigma in ((4, 1.0), (3, float("nan")), (5, float("inf"))):
        with pytest.raises(api.HipCannyError):
            api.gaussian_taps_q8(k, sigma)


def test_header_declares_both_entries_and_the_borders(lib):
    hdr = open(os.path.join(ROOT, "include", "hipcanny.h")).read()
    declared = set(re.findall(r"\b(hc_[a-z0-9_]+)\s*\(", hdr))
    assert {"hc_gaussian_blur_device", "hc_gaussian_taps_q8"} <= declared
    assert declared == set(api.ABI_SYMBOLS) | set(api.ABI_SYMBOLS_HOST)
    assert re.search(r"HC_BORDER_REFLECT_101\s*=\s*0\s*,\s*HC_BORDER_REPLICATE\s*=\s*1", hdr)
    assert (api.BORDER_REFLECT_101, api.BORDER_REPLICATE) == (G.REFLECT_101, G.REPLICATE) == (0, 1)
    assert "not pinned against a build of OpenCV" in hdr[hdr.index("int hc_edge_points_device"):hdr.index("int hc_gaussian_taps_q8")]
