"""The numpy restatement of hc_corner_response_device and hc_good_features_device as include/hipcanny.h states them: int64 window
sums over a replicated border, then the float32 steps one rounded operation at a time (np.float32 scalars and arrays only); keys,
threshold, candidates, the cut at candidate_capacity, the smallest-distance sift.  The GPU tests compare bit for bit with this."""
import math

import numpy as np

MIN_EIGEN, HARRIS = 0, 1


def window_sums(dx, dy, block_size):
    """(a, b, c) int64 planes: the sums of dx^2, dx dy, dy^2 over the centred block_size^2 window, positions clamped to the frame."""
    x, y = np.asarray(dx).astype(np.int64), np.asarray(dy).astype(np.int64)
    r = block_size // 2
    out = []
    for prod in (x * x, x * y, y * y):
        p = np.pad(prod, r, mode="edge")
        h, w = prod.shape
        rows = sum(p[i:i + h, :] for i in range(block_size))
        out.append(sum(rows[:, j:j + w] for j in range(block_size)))
    return out


def corner_response(dx, dy, block_size=3, method=MIN_EIGEN, harris_k=0.04):
    """float32 plane of one frame (2-D int16 dx, dy)."""
    a, b, c = window_sums(dx, dy, block_size)
    fa, fb, fc = a.astype(np.float32), b.astype(np.float32), c.astype(np.float32)
    with np.errstate(all="ignore"):
        if method == MIN_EIGEN:
            half = np.float32(0.5)
            h, g = half * fa, half * fc
            d = h - g
            r = (h + g) - np.sqrt(d * d + fb * fb)
        else:
            k = np.float32(harris_k)
            t = fa + fc
            r = (fa * fc - fb * fb) - (k * t) * t
    assert r.dtype == np.float32
    return r


def keys(plane):
    """uint32 keys of a float32 plane: the bits of v where v > 0, else 0 (an integer test: denormals keep their bits)."""
    bits = np.ascontiguousarray(plane, dtype=np.float32).view(np.uint32)
    return np.where((bits.view(np.int32) > 0) & (bits <= 0x7F800000), bits, np.uint32(0)).astype(np.uint32)


def min_d2(min_distance):
    v = float(min_distance) * float(min_distance)
    return 1 << 62 if v >= 4611686018427387904.0 else int(math.ceil(v))


def threshold_key(k, quality_level):
    """key(t), t = M q one rounded float32 product, M the value with the largest key."""
    m = np.uint32(k.max()).reshape(1).view(np.float32)[0]
    with np.errstate(all="ignore"):
        t = np.float32(m * np.float32(quality_level))
    return int(keys(np.array([t], np.float32))[0])


def candidates(plane, quality_level):
    """(keys, indices) of the candidates of one frame in the order of the rule: key descending, index ascending."""
    k = keys(plane)
    h, w = k.shape
    if w < 3 or h < 3 or int(k.max()) == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.int64)
    tk = threshold_key(k, quality_level)
    c = k[1:-1, 1:-1]
    nb = np.zeros_like(c)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dy, dx) != (1, 1):
                nb = np.maximum(nb, k[dy:dy + h - 2, dx:dx + w - 2])
    ys, xs = np.nonzero((c > tk) & (c >= nb))
    ys, xs = ys + 1, xs + 1
    kk, idx = k[ys, xs], ys.astype(np.int64) * w + xs
    order = np.lexsort((idx, -kk.astype(np.int64)))
    return kk[order], idx[order]


def good_features(plane, quality_level, min_distance, candidate_capacity=4096, corner_capacity=None):
    """(count, corners float32 (min(count, capacity), 2), responses float32) of one float32 frame."""
    w = plane.shape[1]
    kk, idx = candidates(plane, quality_level)
    kk, idx = kk[:candidate_capacity], idx[:candidate_capacity]
    d2 = min_d2(min_distance)
    kept_x, kept_y, kept_k = [], [], []
    for key, i in zip(kk.tolist(), idx.tolist()):
        x, y = i % w, i // w
        if d2 > 0 and kept_x:
            ddx, ddy = np.asarray(kept_x, np.int64) - x, np.asarray(kept_y, np.int64) - y
            if int((ddx * ddx + ddy * ddy).min()) < d2:
                continue
        kept_x.append(x); kept_y.append(y); kept_k.append(key)
    n = len(kept_x)
    m = n if corner_capacity is None else min(n, corner_capacity)
    xy = np.stack([np.asarray(kept_x[:m], np.float32), np.asarray(kept_y[:m], np.float32)], axis=1) if m else np.zeros((0, 2), np.float32)
    return n, xy, np.asarray(kept_k[:m], np.uint32).view(np.float32)
