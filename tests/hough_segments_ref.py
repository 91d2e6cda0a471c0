"""numpy restatement of hc_hough_segments_device / hc_hough_walk_tables, written from the contract in include/hipcanny.h (the form
of cv::cuda::HoughSegmentDetector, restated; not pinned against a build of OpenCV): walk tables, samples, groups, segments.

Every float32 step of the contract is a numpy float32 operation here (the two products and the sum each rounded, no fused
multiply-add); cos / sin are math.cos / math.sin on Python floats (libm, as the library calls them on the host), not numpy's."""
import math

import numpy as np

import hough_ref as R

f32 = np.float32


def _trig(a):
    """(cos, sin) of a Python float as libm gives them: NaN for an infinite or NaN angle, where math.cos raises."""
    return (math.cos(a), math.sin(a)) if math.isfinite(a) else (math.nan, math.nan)


def _div(p, q):
    """p / q in double as C divides: q is never 0 where the rule divides by it, but may be NaN."""
    return p / q if q == q and q != 0 else math.nan


def walk_tables(w, h, rho, theta, min_theta=0.0, max_theta=R.PI):
    """(major int32, slope float32, scale float32), [numangle] each."""
    tt = R.tables(w, h, rho, theta, min_theta, max_theta)[2]
    major, slope, scale = np.empty(len(tt), np.int32), np.empty(len(tt), f32), np.empty(len(tt), f32)
    for n, ang in enumerate(tt):
        c, s = _trig(float(ang))
        if abs(s) >= abs(c):
            major[n], slope[n], scale[n] = 0, f32(_div(-c, s)), f32(_div(1.0, s))
        else:
            major[n], slope[n], scale[n] = 1, f32(_div(-s, c)), f32(_div(1.0, c))
    return major, slope, scale


def samples(w, h, major, slope, scale, line_rho):
    """The walk of one line: (t, m, inside) over t = 0 .. L - 1; m is valid where `inside`."""
    L, M = (h, w) if major else (w, h)
    with np.errstate(all="ignore"):
        t = np.arange(L)
        mf = np.rint(t.astype(f32) * f32(slope) + f32(line_rho) * f32(scale))   # float32 products and sum
        inside = (mf >= 0) & (mf.astype(np.float64) <= M - 1)                  # on the float; False for NaN and the infinities
    m = np.where(inside, mf, 0).astype(np.int64)
    return t, m, inside


def groups_of(steps, max_gap):
    """[(first, last)] of the ascending edge steps, cut where more than max_gap steps lie between two of them."""
    out = []
    for t in steps:
        if out and t - out[-1][1] - 1 <= max_gap:
            out[-1][1] = t
        else:
            out.append([t, t])
    return [(a, b) for a, b in out]


def line_segments(m, w, h, tabs, line, min_length, max_gap, stats=None):
    """The kept segments [(x0, y0, x1, y1)] of one line (rho, theta, votes) on the map m [h, w]; tabs = (tab_theta, major,
    slope, scale).  stats (a dict, optional) counts groups, kept, dropped by min_length and cuts by max_gap."""
    tt, major, slope, scale = tabs
    hit = np.flatnonzero(tt.view(np.uint32) == np.asarray(line[1], f32).view(np.uint32))
    if len(hit) == 0:
        return []
    n = int(hit[0])
    t, mm, inside = samples(w, h, major[n], slope[n], scale[n], line[0])
    x, y = (mm, t) if major[n] else (t, mm)
    edge = inside.copy()
    edge[inside] = np.asarray(m)[y[inside], x[inside]] != 0
    out = []
    gs = groups_of([int(v) for v in t[edge]], max_gap)
    for a, b in gs:
        seg = (int(x[a]), int(y[a]), int(x[b]), int(y[b]))
        if (seg[2] - seg[0]) ** 2 + (seg[3] - seg[1]) ** 2 >= int(min_length) ** 2:   # Python integers: exact
            out.append(seg)
    if stats is not None:
        stats["groups"] = stats.get("groups", 0) + len(gs)
        stats["kept"] = stats.get("kept", 0) + len(out)
        stats["dropped"] = stats.get("dropped", 0) + len(gs) - len(out)
        stats["cuts"] = stats.get("cuts", 0) + max(len(gs) - 1, 0)
    return out


def segments_of(m, lines, w, h, rho, theta, min_theta, max_theta, min_length, max_gap, capacity=None, stats=None):
    """(count, int32 (min(count, capacity), 4) = (x0, y0, x1, y1)) of one frame: its map and the lines to walk (float32 (k, 3),
    already cut to min(line count, line_capacity)), by line in their order, within a line by ascending step."""
    tabs = (R.tables(w, h, rho, theta, min_theta, max_theta)[2], *walk_tables(w, h, rho, theta, min_theta, max_theta))
    segs = []
    for line in np.asarray(lines, f32).reshape(-1, 3):
        segs += line_segments(m, w, h, tabs, line, min_length, max_gap, stats)
    count = len(segs)
    k = count if capacity is None else min(count, int(capacity))
    return count, np.array(segs[:k], np.int32).reshape(k, 4)


def segments_batch(maps, lines, w, h, rho, theta, min_theta, max_theta, min_length, max_gap, capacity=None, stats=None):
    """(uint32 counts [n], [segments per frame]) of a batch of maps and per-frame line lists."""
    res = [segments_of(m, l, w, h, rho, theta, min_theta, max_theta, min_length, max_gap, capacity, stats) for m, l in zip(maps, lines)]
    return np.array([c for c, _ in res], np.uint32), [s for _, s in res]


def draw(m, w, h, rho, theta, min_theta, max_theta, n, line_rho, t0, t1):
    """Sets the walk's own samples of steps t0 .. t1 of the line (line_rho, tab_theta[n]) in the map m: the walk's rasterisation."""
    major, slope, scale = walk_tables(w, h, rho, theta, min_theta, max_theta)
    t, mm, inside = samples(w, h, major[n], slope[n], scale[n], line_rho)
    sel = inside & (t >= t0) & (t <= t1)
    x, y = (mm, t) if major[n] else (t, mm)
    m[y[sel], x[sel]] = 255
    return int(sel.sum())
