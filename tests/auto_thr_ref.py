"""numpy restatement of the automatic threshold rules of hc_auto_thresholds_device (cudacam_amd/csrc/auto_thr.h), from a
uint8 array -- one frame, all channels pooled -- or from its 256-bin histogram.  float64, the operations in the order the
header states them; Python's int -> float conversion rounds to nearest even, as the C cast does.

    median: a = s[(N-1)//2], b = s[N//2] of the sorted samples, v = (a + b) / 2.0 (np.median);
            low = int(max(0.0, (1.0 - sigma) * v)), high = int(min(255.0, (1.0 + sigma) * v))
    otsu:   t* = the smallest t in 0..254 with w0, w1 > 0 whose score (float(d) * float(d)) / (float(w0) * float(w1)),
            d = S * w0 - N * s0 in exact integers, is strictly the largest (0 if there is none);
            high = t*, low = int(ratio * t*)
"""
import numpy as np

MEDIAN, OTSU = 0, 1


def histogram(frame):
    return np.bincount(np.asarray(frame, np.uint8).reshape(-1), minlength=256).astype(np.int64)


def median_value_hist(hist):
    """np.median of the samples a histogram stands for: the mean of sorted samples (N-1)//2 and N//2."""
    cum = np.cumsum(np.asarray(hist, np.int64))
    n = int(cum[-1])
    a = int(np.searchsorted(cum, (n - 1) // 2, side="right"))
    b = int(np.searchsorted(cum, n // 2, side="right"))
    return (float(a) + float(b)) / 2.0


def median_pair(v, sigma):
    v, sigma = float(v), float(sigma)
    return int(max(0.0, (1.0 - sigma) * v)), int(min(255.0, (1.0 + sigma) * v))


def otsu_t_hist(hist):
    h = [int(x) for x in hist]
    n = sum(h)
    s = sum(i * x for i, x in enumerate(h))
    w0 = s0 = 0
    best, best_t = 0.0, -1
    for t in range(255):
        w0 += h[t]
        s0 += t * h[t]
        w1 = n - w0
        if w0 <= 0 or w1 <= 0:
            continue
        d = s * w0 - n * s0
        score = (float(d) * float(d)) / (float(w0) * float(w1))
        if best_t < 0 or score > best:
            best, best_t = score, t
    return max(best_t, 0)


def otsu_pair(t, ratio):
    return int(float(ratio) * float(t)), int(t)


def from_histogram(hist, rule, param):
    if rule in (MEDIAN, "median"):
        return median_pair(median_value_hist(hist), param)
    if rule in (OTSU, "otsu"):
        return otsu_pair(otsu_t_hist(hist), param)
    raise ValueError(f"unknown rule {rule!r}")


def thresholds(frame, rule, param):
    """(low, high) of one uint8 frame ((H,W) or (H,W,C), the channels pooled)."""
    a = np.asarray(frame)
    if a.dtype != np.uint8:
        raise TypeError("frames are uint8")
    if rule in (MEDIAN, "median"):
        v = float(np.median(a))
        assert v == median_value_hist(histogram(a))   # the histogram form above is np.median
        return median_pair(v, param)
    return from_histogram(histogram(a), rule, param)


def normalised(low, high):
    """What hc_set_thresholds makes of a pair on a mode O context: clamped to 0..32767, ordered."""
    lo, hi = (max(0, min(32767, int(v))) for v in (low, high))
    return (hi, lo) if lo > hi else (lo, hi)
