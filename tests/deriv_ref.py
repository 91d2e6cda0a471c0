"""numpy restatement of the derivatives cv::Canny computes before its NMS: Sobel(src, CV_16S, 1, 0 / 0, 1, ksize, scale, 0,
BORDER_REPLICATE) for ksize 3, 5, 7 and -1 (Scharr), with cv::Canny's scale (1, except 1/16 at 7).  Restated from the
published algorithm (OpenCV 4.x modules/imgproc/src/deriv.cpp, canny.cpp) -- not pinned against a build of OpenCV, and
independent of the product: plain int64 index arithmetic, nothing shared with the kernels.

ksize 7: OpenCV scales the smoothing kernel by 1/16, filters in float and converts with saturate_cast<short>(cvRound(v)).
Every intermediate is a multiple of 1/16 below 2^19, so the float path is exact, and the result is the exact integer sum
divided by 16 and rounded half to even (cvRound's rule).  tests/test_deriv_ref_cpu.py checks that claim against a float32
emulation of the separable filter."""
import numpy as np

SMOOTH = {3: [1, 2, 1], 5: [1, 4, 6, 4, 1], 7: [1, 6, 15, 20, 15, 6, 1], -1: [3, 10, 3]}
DERIV = {3: [-1, 0, 1], 5: [-1, -2, 0, 2, 1], 7: [-1, -4, -5, 0, 5, 4, 1], -1: [-1, 0, 1]}
SHIFT = {3: 0, 5: 0, 7: 4, -1: 0}   # the result is the integer sum / 2^SHIFT
KSIZES = (3, 5, 7, -1)


def corr1d(a, taps, axis):
    """Correlation along `axis` with BORDER_REPLICATE: out[i] = sum_j taps[j] * a[clamp(i + j - r)]."""
    r = len(taps) // 2
    n = a.shape[axis]
    out = np.zeros(a.shape, a.dtype)
    for j, t in enumerate(taps):
        idx = np.minimum(np.maximum(np.arange(n) + (j - r), 0), n - 1)
        out = out + t * np.take(a, idx, axis=axis)
    return out


def round_half_even_shift(s, shift):
    """s / 2^shift rounded half to even, in integers."""
    s = np.asarray(s, np.int64)
    if shift == 0:
        return s
    q, rem = s >> shift, s & ((1 << shift) - 1)   # floor and the remainder 0 .. 2^shift - 1
    half = 1 << (shift - 1)
    up = (rem > half) | ((rem == half) & ((q & 1) == 1))
    return q + up


def sums(img, ksize):
    """The unscaled integer sums (Sx, Sy), int64, of one (H,W) or (H,W,C) image (axis 0 = rows, axis 1 = columns)."""
    a = np.asarray(img).astype(np.int64)
    s, d = SMOOTH[ksize], DERIV[ksize]
    return corr1d(corr1d(a, d, 1), s, 0), corr1d(corr1d(a, s, 1), d, 0)


def sobel16(img, ksize):
    """(H,W) or (H,W,C) u8 image -> (dx, dy) int16 of the same shape (CV_16SC1 / CV_16SC3)."""
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim not in (2, 3):
        raise ValueError("sobel16: one (H,W) or (H,W,C) uint8 image")
    sx, sy = sums(a, ksize)
    dx, dy = round_half_even_shift(sx, SHIFT[ksize]), round_half_even_shift(sy, SHIFT[ksize])
    assert max(np.abs(dx).max(initial=0), np.abs(dy).max(initial=0)) <= 32767
    return dx.astype(np.int16), dy.astype(np.int16)


def sobel16_frames(frames, ksize):
    """(n,H,W) or (n,H,W,C) frames -> (dx, dy) int16 of the same shape."""
    out = [sobel16(f, ksize) for f in frames]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
