"""numpy restatement of hc_gaussian_blur_device as include/hipcanny.h states it: a separable K x K correlation (K = 3, 5, 7)
with Q8 taps (256 = 1.0, each <= 256, sum 256), the same along x and y, per channel:

    h = sum_i t[i] * src   along the row     (<= 255 * 256)
    v = sum_j t[j] * h     along the column  (< 2^24)
    out = (v + 32768) >> 16

which is cv::GaussianBlur's fixed-point path for CV_8U (8.8 coefficients, 16.16 accumulator, rounding by adding one half),
restated from the published algorithm (OpenCV 4.x modules/imgproc/src/smooth.dispatch.cpp, fixedpoint.inl.hpp) -- no OpenCV
is installed here, so nothing is pinned against a build of it.  Independent of the product: int64 arithmetic, np.pad for the
borders ("reflect" = BORDER_REFLECT_101, "edge" = BORDER_REPLICATE; np.pad keeps reflecting when the pad is longer than the
axis, as cv::borderInterpolate does), nothing shared with the kernels.  gaussian_taps_q8 restates the taps rule."""
import math

import numpy as np

REFLECT_101, REPLICATE = 0, 1
BORDERS = (REFLECT_101, REPLICATE)
KSIZES = (3, 5, 7)
PAD_MODE = {REFLECT_101: "reflect", REPLICATE: "edge"}
FIXED = {3: [64, 128, 64], 5: [16, 64, 96, 64, 16], 7: [8, 28, 56, 72, 56, 28, 8]}


def gaussian_taps_q8(ksize, sigma):
    if ksize not in FIXED or not math.isfinite(sigma):
        raise ValueError("ksize 3, 5, 7 and a finite sigma")
    if sigma <= 0:
        return list(FIXED[ksize])
    r = ksize // 2
    den = 2.0 * sigma * sigma   # (underflows to 0 for the tiniest sigmas: the centre tap alone)
    g = [1.0 if i == r else (math.exp(-((i - r) ** 2) / den) if den > 0 else 0.0) for i in range(ksize)]
    total = 0.0
    for v in g:
        total += v
    taps, err = [0] * ksize, 0.0
    for i in range(r):   # from the outside inwards, the rounding error diffused to the next tap
        x = 256.0 * (g[i] / total) + err
        v = float(np.rint(x))   # nearbyint: half to even
        err = x - v
        taps[i] = taps[ksize - 1 - i] = int(v)
    taps[r] = 256 - sum(taps)
    return taps


def check_taps(taps):
    t = [int(v) for v in taps]
    if len(t) not in KSIZES or min(t) < 0 or max(t) > 256 or sum(t) != 256:
        raise ValueError(f"taps {t}: 3, 5 or 7 values of 0 .. 256 that sum to 256")
    return t


def corr1d(a, taps, axis, border):
    """Correlation along `axis`: out[i] = sum_j taps[j] * a[border(i + j - r)], int64."""
    r = len(taps) // 2
    pad = [(0, 0)] * a.ndim
    pad[axis] = (r, r)
    p = np.pad(a, pad, mode=PAD_MODE[border])
    n = a.shape[axis]
    out = np.zeros(a.shape, np.int64)
    for j, t in enumerate(taps):
        out += t * np.take(p, np.arange(j, j + n), axis=axis)
    return out


def blur(img, taps, border=REFLECT_101):
    """One (H,W) or (H,W,C) u8 image -> the blurred u8 image of the same shape."""
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim not in (2, 3):
        raise ValueError("blur: one (H,W) or (H,W,C) uint8 image")
    t = check_taps(taps)
    h = corr1d(a.astype(np.int64), t, 1, border)
    assert h.max(initial=0) <= 65280
    v = corr1d(h, t, 0, border)
    assert v.max(initial=0) < 1 << 24
    return ((v + 32768) >> 16).astype(np.uint8)


def blur_frames(frames, taps, border=REFLECT_101):
    """(n,H,W) or (n,H,W,C) frames -> blurred frames of the same shape."""
    return np.stack([blur(f, taps, border) for f in frames])


def gauss_blur_ref(frames, ksize, sigma, border=REFLECT_101):
    return blur_frames(frames, gaussian_taps_q8(ksize, sigma), border)
