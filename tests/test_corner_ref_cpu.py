"""Anchors tests/corner_ref.py (the numpy restatement of hc_corner_response_device and hc_good_features_device) without a GPU:
a second, independent per-pixel double-loop restatement on small random planes with extreme values; the window sums against
scipy.ndimage.correlate on int64 with mode="nearest"; exact invariants (flat frame, vertical step edge, the four corners of a
bright square and their symmetries); the select / order / sift rules against a plain sorted() plus loop model on planes with many
equal keys."""
import math
import struct

import numpy as np
import pytest

import corner_ref as R


def _f32(v):
    return np.float32(v)


def _loop_response(dx, dy, B, method, k):
    """per pixel, Python ints for the sums, one np.float32 operation per step"""
    h, w = dx.shape
    r = B // 2
    out = np.zeros((h, w), np.float32)
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                a = b = c = 0
                for j in range(-r, r + 1):
                    for i in range(-r, r + 1):
                        yy, xx = min(max(y + j, 0), h - 1), min(max(x + i, 0), w - 1)
                        gx, gy = int(dx[yy, xx]), int(dy[yy, xx])
                        a += gx * gx; b += gx * gy; c += gy * gy
                # int -> float32 in one rounding: through the exact double (|sum| < 2^53)
                fa, fb, fc = _f32(float(a)), _f32(float(b)), _f32(float(c))
                if method == R.MIN_EIGEN:
                    hh, g = _f32(0.5) * fa, _f32(0.5) * fc
                    d = _f32(hh - g)
                    out[y, x] = _f32(_f32(hh + g) - np.sqrt(_f32(_f32(d * d) + _f32(fb * fb))))
                else:
                    kk, t = _f32(k), _f32(fa + fc)
                    out[y, x] = _f32(_f32(_f32(fa * fc) - _f32(fb * fb)) - _f32(_f32(kk * t) * t))
    return out


def _planes(rng, h, w, kind):
    if kind == "small":
        return rng.integers(-300, 300, (h, w)).astype(np.int16), rng.integers(-300, 300, (h, w)).astype(np.int16)
    if kind == "full":
        return rng.integers(-32768, 32768, (h, w)).astype(np.int16), rng.integers(-32768, 32768, (h, w)).astype(np.int16)
    ext = np.array([-32768, 32767, 0, -1, 1], np.int16)
    return ext[rng.integers(0, 5, (h, w))], ext[rng.integers(0, 5, (h, w))]


@pytest.mark.parametrize("B", [3, 5, 7])
@pytest.mark.parametrize("method", [R.MIN_EIGEN, R.HARRIS])
def test_response_against_the_per_pixel_loop(B, method):
    rng = np.random.default_rng(100 * B + method)
    for kind in ("small", "full", "extreme"):
        for (h, w) in ((1, 1), (2, 9), (9, 7), (B - 1, B)):
            dx, dy = _planes(rng, h, w, kind)
            for k in (0.0, 0.04, 0.25):
                got, want = R.corner_response(dx, dy, B, method, k), _loop_response(dx, dy, B, method, k)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (kind, h, w, k)
                if method == R.MIN_EIGEN:
                    break


@pytest.mark.parametrize("B", [3, 5, 7])
def test_sums_against_scipy(B):
    from scipy import ndimage   # (required: a missing scipy is a failure of this anchor, not a skip)
    rng = np.random.default_rng(B)
    dx, dy = _planes(rng, 23, 31, "full")
    x, y = dx.astype(np.int64), dy.astype(np.int64)
    ones = np.ones((B, B), np.int64)
    for got, prod in zip(R.window_sums(dx, dy, B), (x * x, x * y, y * y)):
        assert got.dtype == np.int64 and np.array_equal(got, ndimage.correlate(prod, ones, mode="nearest"))
    c = np.full((9, 9), -32768, np.int16)
    assert int(R.window_sums(c, c, 7)[0].max()) == 49 << 30


def test_flat_frame_gives_zero():
    z = np.full((12, 17), 5, np.int16) * 0
    for B in (3, 5, 7):
        for m in (R.MIN_EIGEN, R.HARRIS):
            assert not R.corner_response(z, z, B, m).view(np.uint32).any()


def test_vertical_step_edge():
    img = np.zeros((20, 24), np.int32); img[:, 12:] = 200
    dx = np.zeros_like(img); dx[:, 1:-1] = img[:, 2:] - img[:, :-2]
    dx, dy = dx.astype(np.int16), np.zeros(img.shape, np.int16)
    for B in (3, 5, 7):
        assert not R.corner_response(dx, dy, B, R.MIN_EIGEN).view(np.uint32).any()   # exactly +0.0 everywhere
        assert (R.corner_response(dx, dy, B, R.HARRIS, 0.04) <= 0).all()


def _sobel3(img):
    p = np.pad(img.astype(np.int32), 1, mode="edge")
    gx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    gy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    return gx.astype(np.int16), gy.astype(np.int16)


def test_bright_square_has_four_corners_and_keeps_its_symmetries():
    n = 41
    img = np.zeros((n, n), np.uint8); img[12:29, 12:29] = 255   # symmetric in a symmetric frame
    # the eight symmetries of the frame as maps of a point (x, y)
    maps = [lambda x, y: (x, y), lambda x, y: (n - 1 - x, y), lambda x, y: (x, n - 1 - y), lambda x, y: (n - 1 - x, n - 1 - y),
            lambda x, y: (y, x), lambda x, y: (n - 1 - y, x), lambda x, y: (y, n - 1 - x), lambda x, y: (n - 1 - y, n - 1 - x)]
    gx, gy = _sobel3(img)
    for m in (R.MIN_EIGEN, R.HARRIS):
        resp = R.corner_response(gx, gy, 3, m, 0.04)
        cnt, xy, q = R.good_features(resp, 0.5, 2.0)
        assert cnt == 4, (m, xy)
        pts = {(int(x), int(y)) for x, y in xy}
        for vx in (12, 28):
            for vy in (12, 28):
                assert any(abs(x - vx) <= 2 and abs(y - vy) <= 2 for x, y in pts), (pts, vx, vy)
        for t, f in enumerate(maps):
            assert {f(x, y) for x, y in pts} == pts, (m, t, pts)   # each symmetry sends the set onto itself
    # ... and on a frame that is NOT symmetric (the square off centre, a second one beside it) the corners move with the image
    img = np.zeros((n, n), np.uint8); img[5:16, 8:23] = 255; img[24:35, 20:27] = 200
    gx, gy = _sobel3(img)
    base = {(int(x), int(y)) for x, y in R.good_features(R.corner_response(gx, gy, 3, R.MIN_EIGEN), 0.3, 2.0)[1]}
    assert len(base) == 8
    for t, (im, f) in enumerate(((img[:, ::-1], maps[1]), (img[::-1], maps[2]), (img[::-1, ::-1], maps[3]), (img.T, maps[4]))):
        gx, gy = _sobel3(np.ascontiguousarray(im))
        got = {(int(x), int(y)) for x, y in R.good_features(R.corner_response(gx, gy, 3, R.MIN_EIGEN), 0.3, 2.0)[1]}
        assert got == {f(x, y) for x, y in base}, (t, got, base)


def _model(plane, q, md, cap):
    """sorted() plus loop, keys by struct"""
    h, w = plane.shape
    def key(v):
        b = struct.unpack("<I", struct.pack("<f", v))[0]
        return b if (0 < b <= 0x7F800000) else 0
    k = [[key(float(plane[y, x])) for x in range(w)] for y in range(h)]
    M = max(max(r) for r in k)
    if M == 0 or w < 3 or h < 3:
        return []
    mval = struct.unpack("<f", struct.pack("<I", M))[0]
    with np.errstate(all="ignore"):
        tk = key(float(np.float32(np.float32(mval) * np.float32(q))))
    cands = []
    for y in range(1, h - 1):
        for x in range(1, w - 1):
            if k[y][x] > tk and all(k[y][x] >= k[y + j][x + i] for j in (-1, 0, 1) for i in (-1, 0, 1)):
                cands.append((-k[y][x], y * w + x))
    cands = sorted(cands)[:cap]
    d2 = R.min_d2(md)
    kept = []
    for nk, i in cands:
        x, y = i % w, i // w
        if all((x - a) ** 2 + (y - b) ** 2 >= d2 for a, b, _ in kept):
            kept.append((x, y, -nk))
    return kept


@pytest.mark.parametrize("seed", range(6))
def test_select_order_sift_against_the_sorted_model(seed):
    rng = np.random.default_rng(seed)
    h, w = 19 + seed, 23
    levels = np.array([0.0, 1.0, 1.0, 2.0, 2.0000002, 3.5, -1.0, np.nan, 1e-41], np.float32)   # many equal keys, a denormal, junk
    plane = levels[rng.integers(0, len(levels), (h, w))]
    for q, md, cap in ((0.01, 0.0, 4096), (0.2, 1.5, 4096), (0.3, 3.0, 17), (0.01, 0.0, 5), (1.0, 0.0, 10), (0.01, 100.0, 64)):
        want = _model(plane, q, md, cap)
        cnt, xy, qual = R.good_features(plane, q, md, cap)
        assert cnt == len(want)
        assert [(int(x), int(y)) for x, y in xy] == [(a, b) for a, b, _ in want]
        assert qual.view(np.uint32).tolist() == [kk for _, _, kk in want]
        c2, xy2, q2 = R.good_features(plane, q, md, cap, corner_capacity=3)
        assert c2 == cnt and len(xy2) == min(cnt, 3) and np.array_equal(xy2, xy[:3])


def test_keys_and_min_d2():
    v = np.array([0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, 1e-45, 1.0], np.float32)
    assert R.keys(v).tolist() == [0, 0, 0, 0, 0x7F800000, 0, 1, 0x3F800000]
    assert R.min_d2(0) == 0 and R.min_d2(1) == 1 and R.min_d2(math.sqrt(2)) == 3 and R.min_d2(1e9) == 10 ** 18
    assert R.min_d2(2.0 ** 31) == 1 << 62 and R.min_d2(1e300) == 1 << 62 and R.min_d2(2.0 ** 30.5) < 1 << 62
