"""numpy restatement of hc_hough_lines_device / hc_hough_tables, written from the contract in include/hipcanny.h (cv::HoughLines
with srn = stn = 0, restated; not pinned against a build of OpenCV): geometry, tables, votes, peaks, order and lines.

Every float32 step of the contract is a numpy float32 operation here (products and the sum each rounded, no fused multiply-add);
cos / sin are math.cos / math.sin on Python floats (libm, as the library calls them on the host), not numpy's."""
import math

import numpy as np

PI = 3.1415926535897932384626433832795
f32 = np.float32


def geometry(w, h, rho, theta, min_theta=0.0, max_theta=PI):
    """(numangle, numrho)."""
    numangle = int(math.floor((max_theta - min_theta) / theta)) + 1
    if numangle > 1 and abs(PI - (numangle - 1) * theta) < theta / 2:
        numangle -= 1
    numrho = round((2.0 * (w + h) + 1.0) / rho)   # Python rounds a float half to even, exactly
    return numangle, int(numrho)


def tables(w, h, rho, theta, min_theta=0.0, max_theta=PI):
    """(tab_cos, tab_sin, tab_theta), float32 [numangle] each."""
    numangle, _ = geometry(w, h, rho, theta, min_theta, max_theta)
    irho = f32(1.0) / f32(rho)
    ang, step = f32(min_theta), f32(theta)
    tc, ts, tt = np.empty(numangle, f32), np.empty(numangle, f32), np.empty(numangle, f32)
    for n in range(numangle):
        tc[n] = f32(math.cos(float(ang)) * float(irho))
        ts[n] = f32(math.sin(float(ang)) * float(irho))
        tt[n] = ang
        ang = f32(ang + step)
    return tc, ts, tt


def accumulate(points, numangle, numrho, tab_cos, tab_sin):
    """The padded accumulator int32 [numangle + 2][numrho + 2] of a list of (x, y)."""
    acc = np.zeros((numangle + 2, numrho + 2), np.int32)
    pts = np.asarray(points, np.int32).reshape(-1, 2)
    x, y = pts[:, 0].astype(f32), pts[:, 1].astype(f32)
    half = int((numrho - 1) / 2)   # C's integer division: towards zero
    for n in range(numangle):
        px, py = x * tab_cos[n], y * tab_sin[n]   # float32 each
        r = np.rint(px + py)                      # float32 sum, half to even
        r = r[np.isfinite(r)].astype(np.int64) + half
        r = r[(r >= -1) & (r <= numrho)]
        acc[n + 1] += np.bincount(r + 1, minlength=numrho + 2).astype(np.int32)
    return acc


def peaks(acc, numangle, numrho, threshold):
    """(votes, n, r) of every peak, in cv::HoughLines' order: votes descending, accumulator index ascending."""
    a = acc[1:numangle + 1, 1:numrho + 1]
    m = ((a > threshold) & (a > acc[1:numangle + 1, 0:numrho]) & (a >= acc[1:numangle + 1, 2:numrho + 2])
         & (a > acc[0:numangle, 1:numrho + 1]) & (a >= acc[2:numangle + 2, 1:numrho + 1]))
    n, r = np.nonzero(m)
    votes = a[n, r].astype(np.int64)
    index = (n + 1) * (numrho + 2) + r + 1
    order = np.lexsort((index, -votes))
    return votes[order], n[order], r[order]


def hough_lines(points, w, h, rho, theta, threshold, min_theta=0.0, max_theta=PI, capacity=None):
    """(count, float32 (min(count, capacity), 3) = (rho, theta, votes)) of one frame's point list."""
    numangle, numrho = geometry(w, h, rho, theta, min_theta, max_theta)
    tc, ts, tt = tables(w, h, rho, theta, min_theta, max_theta)
    votes, n, r = peaks(accumulate(points, numangle, numrho, tc, ts), numangle, numrho, threshold)
    count = len(votes)
    k = count if capacity is None else min(count, int(capacity))
    out = np.empty((k, 3), f32)
    out[:, 0] = (r[:k].astype(f32) - f32(numrho - 1) * f32(0.5)) * f32(rho)
    out[:, 1] = tt[n[:k]]
    out[:, 2] = votes[:k].astype(f32)
    return count, out


def hough_lines_batch(lists, w, h, rho, theta, threshold, min_theta=0.0, max_theta=PI, capacity=None):
    """(uint32 counts [n], [lines per frame]) of a batch of point lists."""
    res = [hough_lines(p, w, h, rho, theta, threshold, min_theta, max_theta, capacity) for p in lists]
    return np.array([c for c, _ in res], np.uint32), [l for _, l in res]


def points_of(m):
    """cv::findNonZero: (x, y) int32 in raster order."""
    ys, xs = np.nonzero(np.asarray(m))
    return np.stack([xs, ys], axis=1).astype(np.int32)
