"""numpy restatement of Mode O beyond aperture 3: cv::Canny(img, low, high, apertureSize 3 / 5, L2gradient) and
cv::Canny(dx, dy, edges, low, high, L2gradient) (OpenCV 4.x modules/imgproc/src/canny.cpp, restated from the published
algorithm -- not pinned against a build of OpenCV).  Independent of the oracle's C code: int32 two's-complement
arithmetic (wrap-around) done explicitly in int64, the flood as 8-connected components (scipy.ndimage.label)."""
import numpy as np
from scipy import ndimage

TG22 = 13573   # (int)(tan(22.5 deg) * 2^15 + 0.5)
SMOOTH = {3: [1, 2, 1], 5: [1, 4, 6, 4, 1]}
DERIV = {3: [-1, 0, 1], 5: [-1, -2, 0, 2, 1]}


def wrap32(a):
    a = np.asarray(a, np.int64)
    return ((a + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _corr1d(img, taps, axis):
    """Correlation along `axis` with BORDER_REPLICATE (indices clamped into the image)."""
    r = len(taps) // 2
    n = img.shape[axis]
    out = np.zeros(img.shape, np.int64)
    for j, t in enumerate(taps):
        if t:
            idx = np.clip(np.arange(n) + j - r, 0, n - 1)
            out += t * np.take(img, idx, axis=axis)
    return out


def sobel_o(img, ksize=3):
    """Sobel(src, CV_16S, ksize, scale 1, BORDER_REPLICATE) of a (H,W) or (H,W,C) u8 image -> (dx, dy) int32, same shape."""
    a = np.asarray(img).astype(np.int64)
    s, d = SMOOTH[ksize], DERIV[ksize]
    dx = _corr1d(_corr1d(a, d, 1), s, 0)
    dy = _corr1d(_corr1d(a, s, 1), d, 0)
    return dx.astype(np.int32), dy.astype(np.int32)


def thresholds(low, high, l2):
    """canny.cpp's threshold handling (as the oracle): ordered, L2: capped at 32767 and squared, floored."""
    low, high = float(low), float(high)
    if low > high:
        low, high = high, low
    if l2:
        low, high = min(low, 32767.0), min(high, 32767.0)
        low = low * low if low > 0 else low
        high = high * high if high > 0 else high
    return int(np.floor(low)), int(np.floor(high))


def canny_o_from_gradients(dx, dy, low, high, l2=False, premap=False):
    """Everything of Mode O after the Sobel: dx, dy int (H,W) or (H,W,C) -> u8 edge map (0 / 255); with premap=True also
    the map before the flood (255 seed, 128 candidate, 0 none)."""
    dx, dy = np.asarray(dx, np.int64), np.asarray(dy, np.int64)
    if dx.ndim == 2:
        dx, dy = dx[..., None], dy[..., None]
    lo, hi = thresholds(low, high, l2)
    mags = wrap32(dx * dx + dy * dy) if l2 else np.abs(dx) + np.abs(dy)
    # first channel with the largest magnitude (strictly larger replaces)
    m, X, Y = mags[..., 0].copy(), dx[..., 0].copy(), dy[..., 0].copy()
    for k in range(1, mags.shape[-1]):
        t = mags[..., k] > m
        m[t], X[t], Y[t] = mags[..., k][t], dx[..., k][t], dy[..., k][t]
    h, w = m.shape
    P = np.zeros((h + 2, w + 2), np.int64)   # m = 0 outside the image
    P[1:-1, 1:-1] = m

    def nb(dr, dc):
        return P[1 + dr:1 + dr + h, 1 + dc:1 + dc + w]

    x = np.abs(X)
    y = np.abs(Y) << 15
    tg22x = wrap32(x * TG22)
    tg67x = wrap32(tg22x + (x << 16))
    horiz = y < tg22x
    vert = ~horiz & (y > tg67x)
    diag = ~horiz & ~vert
    neg = (X ^ Y) < 0
    kh = (m > nb(0, -1)) & (m >= nb(0, 1))
    kv = (m > nb(-1, 0)) & (m >= nb(1, 0))
    kp = (m > nb(-1, -1)) & (m > nb(1, 1))
    kn = (m > nb(-1, 1)) & (m > nb(1, -1))
    keep = (m > lo) & ((horiz & kh) | (vert & kv) | (diag & ~neg & kp) | (diag & neg & kn))
    strong = keep & (m > hi)
    lab, _ = ndimage.label(keep, structure=np.ones((3, 3), bool))
    seeded = np.unique(lab[strong])
    edges = np.isin(lab, seeded[seeded > 0]) & keep
    out = np.where(edges, 255, 0).astype(np.uint8)
    if premap:
        pre = np.where(strong, 255, np.where(keep, 128, 0)).astype(np.uint8)
        return out, pre
    return out


def canny_o(img, low, high, ksize=3, l2=False, premap=False):
    """cv::Canny(img, low, high, ksize, l2)."""
    dx, dy = sobel_o(img, ksize)
    return canny_o_from_gradients(dx, dy, low, high, l2, premap)
