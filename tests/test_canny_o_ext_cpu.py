"""Mode O beyond aperture 3 (HC_OPT_APERTURE 5, hc_run_gradients_device), checked on the CPU: the numpy restatement
the GPU tests compare against is anchored to the committed oracle at aperture 3, its 5x5 Sobel to a brute-force
correlation, and the library / header carry the new surface."""
import os
import re

import numpy as np
import pytest

from cudacam_amd import api, synth
import canny_o_ext_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rgb(w, h, seed):
    return np.stack([synth.natural(w, h, seed), synth.noise(w, h, seed + 1), synth.natural(w, h, seed + 2)[::-1].copy()], -1)


ANCHOR_IMAGES = [
    ("one_px", lambda: np.array([[200]], np.uint8), 50, 150),
    ("two", lambda: synth.noise(2, 2, 3), 10, 30),
    ("five", lambda: synth.noise(5, 5, 4), 10, 30),
    ("natural_640x480", lambda: synth.natural(640, 480, 1), 50, 150),
    ("noise_641x479", lambda: synth.noise(641, 479, 2), 100, 300),
    ("noise_low", lambda: synth.noise(333, 222, 5), 0, 40),
    ("natural_31x33", lambda: synth.natural(31, 33, 3), 20, 60),
    ("flat255", lambda: synth.flat(300, 70, 255), 50, 150),
    ("step_v", lambda: synth.steps(260, 64, 255, "vertical"), 50, 150),
    ("step_h", lambda: synth.steps(100, 90, 240, "horizontal"), 50, 150),
    ("step_d", lambda: synth.steps(250, 250, 120, "diagonal"), 50, 150),
    ("serpentine", lambda: synth.serpentine(500, 300, amp=30, seed_amp=200), 50, 150),
    ("swapped", lambda: synth.natural(200, 100, 8), 150, 50),
    ("rgb_101x77", lambda: _rgb(101, 77, 11), 50, 150),
    ("rgb_7x3", lambda: _rgb(7, 3, 12), 20, 60),
    ("rgb_step", lambda: np.stack([synth.steps(64, 40, 200, "diagonal")] * 3, -1), 50, 150),
]


@pytest.mark.parametrize("l2", [False, True], ids=["L1", "L2"])
@pytest.mark.parametrize("name,make,low,high", ANCHOR_IMAGES, ids=[m[0] for m in ANCHOR_IMAGES])
def test_restatement_matches_oracle_at_aperture3(oracle, name, make, low, high, l2):
    """canny_o_from_gradients(sobel_o(img, 3)) == oracle.canny_o / canny_o_stages, bit for bit (32 cases)."""
    img = make()
    dx, dy = X.sobel_o(img, 3)
    got, got_pre = X.canny_o_from_gradients(dx, dy, low, high, l2, premap=True)
    want, want_pre = oracle.canny_o_stages(img, low, high, l2gradient=l2)
    assert np.array_equal(got_pre, want_pre), f"{name}: premap differs"
    assert np.array_equal(got, want), f"{name}: edges differ"
    assert np.array_equal(got, oracle.canny_o(img, low, high, l2gradient=l2))


def _brute_sobel5(img):
    s, d = [1, 4, 6, 4, 1], [-1, -2, 0, 2, 1]
    a = img.astype(np.int64)
    h, w = a.shape[:2]
    dx = np.zeros(a.shape, np.int64)
    dy = np.zeros(a.shape, np.int64)
    for r in range(h):
        for c in range(w):
            for i in range(-2, 3):
                for j in range(-2, 3):
                    p = a[min(max(r + i, 0), h - 1), min(max(c + j, 0), w - 1)]
                    dx[r, c] += s[i + 2] * d[j + 2] * p
                    dy[r, c] += d[i + 2] * s[j + 2] * p
    return dx, dy


@pytest.mark.parametrize("img", [synth.noise(13, 9, 7), synth.natural(17, 12, 2), synth.noise(1, 1, 3), synth.noise(3, 6, 4),
                                 np.stack([synth.noise(6, 5, 8)] * 3, -1)], ids=["noise13x9", "natural17x12", "1x1", "3x6", "rgb6x5"])
def test_sobel5_matches_brute_force(img):
    dx, dy = X.sobel_o(img, 5)
    bx, by = _brute_sobel5(img)
    assert np.array_equal(dx, bx) and np.array_equal(dy, by)


def test_sobel5_range_and_step_kat():
    img = np.zeros((9, 12), np.uint8)
    img[:, 6:] = 255                    # vertical 0 | 255 step between columns 5 and 6
    dx, dy = X.sobel_o(img, 5)
    assert list(dx[4]) == [0, 0, 0, 0, 4080, 12240, 12240, 4080, 0, 0, 0, 0]
    assert not dy.any()
    edges = X.canny_o(img, 50, 150, ksize=5)
    assert np.array_equal(np.nonzero(edges.any(0))[0], [5]), "one pixel wide, at column c (c + 1 fails m > left)"
    # the extremes: a checkerboard of 0 / 255 in 2-column bands reaches |dx| = 12240 but not beyond
    cb = np.zeros((20, 20), np.uint8)
    cb[:, 2:4] = cb[:, 6:8] = 255
    for im in (cb, cb.T.copy(), synth.noise(64, 64, 1)):
        gx, gy = X.sobel_o(im, 5)
        assert np.abs(gx).max() <= 12240 and np.abs(gy).max() <= 12240


def test_wrap_rules():
    """The two int32 wrap-arounds of full-range int16 gradients."""
    # L2 magnitude wraps to INT_MIN only for dx = dy = -32768: never above the low threshold
    assert X.wrap32(2 * 32768 * 32768) == -(1 << 31)
    assert X.wrap32(32767 * 32767 + 32768 * 32768) > 0
    # tg67x = x * TG22 + (x << 16) wraps from |dx| = 27146 on: such a pixel that is not horizontal is vertical, not diagonal
    for x, wraps in ((27145, False), (27146, True), (32768, True)):
        assert (X.wrap32(x * X.TG22 + (x << 16)) < 0) == wraps
    dx = np.zeros((3, 5), np.int16)
    dy = np.zeros((3, 5), np.int16)
    dx[1, 2], dy[1, 2] = 30000, 30000      # |dy| = |dx|: diagonal without the wrap, vertical with it
    dy[0, 2], dx[0, 2] = 30000, 30000       # diagonal neighbours are 0 and would keep it; the upper one is as strong (m > up fails)
    got = X.canny_o_from_gradients(dx, dy, 10, 20, False)
    assert got[1, 2] == 0


def test_library_exports_gradient_entry_and_header_declares_aperture():
    """The new surface: fails on a library / header without it."""
    hdr = open(os.path.join(ROOT, "include", "hipcanny.h")).read()
    m = re.search(r"HC_OPT_APERTURE\s*=\s*(\d+)", hdr)
    assert m, "hipcanny.h does not declare HC_OPT_APERTURE"
    assert int(m.group(1)) == api.OPT_APERTURE
    assert re.search(r"\bint\s+hc_run_gradients_device\s*\(", hdr)
    assert "hc_run_gradients_device" in api.ABI_SYMBOLS
    lib = api.load_library()
    assert hasattr(lib, "hc_run_gradients_device")
    # argument checks that need no device: a null context is refused
    assert lib.hc_run_gradients_device(None, None, None, 0, 0, None, 0, 0, 1) == -1
    src = open(os.path.join(ROOT, "cudacam_amd", "build.py")).read()
    assert "front_o_ext.hip" in src
