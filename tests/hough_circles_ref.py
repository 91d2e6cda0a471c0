"""numpy restatement of hc_hough_circles_device / hc_hough_circle_geometry, written from the contract in include/hipcanny.h (the
form of cv::cuda::HoughCirclesDetector, restated; not pinned against a build of OpenCV): geometry, centre votes, centres, the
smallest-distance rule, radius histograms, circles.

Every float32 step of the contract is one numpy float32 operation here (each product, quotient, sum and square root rounded, no
fused multiply-add); rint is np.rint (half to even); the fixed-point walk is int64 arithmetic on values the contract keeps
inside int32.  `stats` (a dict, optional) counts what the GPU tests demand of their inputs: rays cut by the accumulator's
border, centres dropped by the smallest distance, centres with two and more radii, ties in the votes of the ranked centres."""
import math

import numpy as np

f32 = np.float32
MAX_CENTRES, MAX_HIST, COORD_LIMIT = 4096, 4096, 1 << 20


def geometry(w, h, dp, min_dist, min_radius, max_radius):
    """(AW, AH, min_d2); ValueError for what hc_hough_circle_geometry refuses."""
    dp, min_dist = float(dp), float(min_dist)
    if w < 1 or h < 1 or not math.isfinite(dp) or dp < 1 or not math.isfinite(min_dist) or min_dist < 0:
        raise ValueError("geometry")
    if min_radius < 1 or max_radius < min_radius or max_radius - min_radius + 3 > MAX_HIST or w + max_radius >= COORD_LIMIT or h + max_radius >= COORD_LIMIT:
        raise ValueError("radii")
    with np.errstate(all="ignore"):
        idp = f32(1.0) / f32(dp)
        aw, ah = math.ceil(float(f32(w) * idp)), math.ceil(float(f32(h) * idp))
    if aw < 1 or ah < 1 or (aw + 2) * (ah + 2) >= 1 << 31:
        raise ValueError("accumulator")
    md = min_dist / dp
    v = md * md
    return aw, ah, (1 << 62) if v >= 2.0 ** 62 else math.ceil(v)


def _inside(points, w, h):
    """The points that take part: int64 (k, 2) with 0 <= x < w, 0 <= y < h, in their order."""
    p = np.asarray(points, np.int64).reshape(-1, 2)
    return p[(p[:, 0] >= 0) & (p[:, 0] < w) & (p[:, 1] >= 0) & (p[:, 1] < h)]


def rays(x, y, vx, vy, dp):
    """(x0, y0, sx, sy) int64 arrays of points inside the frame with gradients (vx, vy) not both 0."""
    idp = f32(1.0) / f32(dp)
    vx, vy = np.asarray(vx, np.int64), np.asarray(vy, np.int64)
    mag = np.sqrt((vx * vx + vy * vy).astype(np.uint32).astype(f32))
    k = f32(1024.0)
    x0 = np.rint((np.asarray(x).astype(f32) * idp) * k).astype(np.int64)
    y0 = np.rint((np.asarray(y).astype(f32) * idp) * k).astype(np.int64)
    sx = np.rint(((vx.astype(f32) * idp) * k) / mag).astype(np.int64)
    sy = np.rint(((vy.astype(f32) * idp) * k) / mag).astype(np.int64)
    return x0, y0, sx, sy


def accumulate(points, dx, dy, w, h, dp, min_radius, max_radius, stats=None):
    """The padded accumulator int32 [AH + 2][AW + 2] of one frame: its point list (k, 2) and its int16 planes [h, w]."""
    aw, ah, _ = geometry(w, h, dp, 0.0, min_radius, max_radius)
    acc = np.zeros((ah + 2, aw + 2), np.int64)
    p = _inside(points, w, h)
    vx, vy = np.asarray(dx)[p[:, 1], p[:, 0]].astype(np.int64), np.asarray(dy)[p[:, 1], p[:, 0]].astype(np.int64)
    go = (vx != 0) | (vy != 0)
    x0, y0, sx, sy = rays(p[go, 0], p[go, 1], vx[go], vy[go], dp)
    for d in (1, -1):
        x1, y1 = x0 + d * min_radius * sx, y0 + d * min_radius * sy
        assert np.abs(x1).max(initial=0) < 1 << 31 and np.abs(y1).max(initial=0) < 1 << 31
        alive = np.ones(len(x0), bool)
        for _ in range(min_radius, max_radius + 1):
            x2, y2 = x1 >> 10, y1 >> 10
            ok = alive & (x2 >= 0) & (x2 < aw) & (y2 >= 0) & (y2 < ah)
            if stats is not None:
                stats["cut_rays"] = stats.get("cut_rays", 0) + int((alive & ~ok).sum())
            alive = ok
            if not alive.any():
                break
            np.add.at(acc, (y2[alive] + 1, x2[alive] + 1), 1)
            x1, y1 = x1 + d * sx, y1 + d * sy
    return acc.astype(np.int32)


def centres(acc, threshold):
    """int64 (k, 3) = (votes, cx, cy) of every centre of a padded accumulator, votes descending, ties by ascending index."""
    a = np.asarray(acc, np.int64)
    mid = a[1:-1, 1:-1]
    pk = (mid > threshold) & (mid > a[:-2, 1:-1]) & (mid >= a[2:, 1:-1]) & (mid > a[1:-1, :-2]) & (mid >= a[1:-1, 2:])
    cy, cx = np.nonzero(pk)   # (index order: the row first)
    votes = mid[cy, cx]
    order = np.argsort(-votes, kind="stable")
    return np.stack([votes[order], cx[order], cy[order]], axis=1).reshape(-1, 3)


def sift(ranked, min_d2, centre_capacity=MAX_CENTRES, stats=None):
    """The centres the smallest distance keeps of the first centre_capacity ranked ones, in their order."""
    ranked = np.asarray(ranked, np.int64).reshape(-1, 3)[:centre_capacity]
    kept, kxy, nk = [], np.zeros((len(ranked), 2), np.int64), 0
    for v, cx, cy in ranked.tolist():
        d = kxy[:nk] - (cx, cy)   # (int64: coordinates below 2^20, squares below 2^41)
        if nk == 0 or int((d * d).sum(axis=1).min()) >= min_d2:
            kept.append((v, cx, cy))
            kxy[nk] = (cx, cy)
            nk += 1
    if stats is not None:
        stats["dropped"] = stats.get("dropped", 0) + len(ranked) - len(kept)
        stats["ties"] = stats.get("ties", 0) + int((ranked[1:, 0] == ranked[:-1, 0]).sum())
    return np.array(kept, np.int64).reshape(-1, 3)


def histogram(points, w, h, cx, cy, dp, min_radius, max_radius):
    """(fx, fy, hist int64 [max_radius - min_radius + 3]) of one centre over the frame's points."""
    p = _inside(points, w, h)
    fx, fy = (f32(cx) + f32(0.5)) * f32(dp), (f32(cy) + f32(0.5)) * f32(dp)
    ddx, ddy = fx - p[:, 0].astype(f32), fy - p[:, 1].astype(f32)
    rad = np.sqrt(ddx * ddx + ddy * ddy)
    assert rad.dtype == f32
    sel = (rad >= f32(min_radius)) & (rad <= f32(max_radius))
    idx = np.rint(rad[sel] - f32(min_radius)).astype(np.int64) + 1
    return fx, fy, np.bincount(idx, minlength=max_radius - min_radius + 3)


def radii(points, w, h, cx, cy, dp, threshold, min_radius, max_radius):
    """float32 (k, 4) = (fx, fy, radius, votes) of one centre, by ascending radius."""
    fx, fy, hist = histogram(points, w, h, cx, cy, dp, min_radius, max_radius)
    hh = hist[1:-1]
    i = np.flatnonzero((hh >= threshold) & (hh > hist[:-2]) & (hh >= hist[2:]))
    out = np.empty((len(i), 4), f32)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = fx, fy, (i + min_radius).astype(f32), hh[i].astype(f32)
    return out


def circles_of(points, dx, dy, w, h, dp, min_dist, threshold, min_radius, max_radius, centre_capacity=MAX_CENTRES, capacity=None, stats=None):
    """(count, float32 (min(count, capacity), 4)) of one frame: its point list (already cut to min(count, point_capacity))."""
    _, _, min_d2 = geometry(w, h, dp, min_dist, min_radius, max_radius)
    acc = accumulate(points, dx, dy, w, h, dp, min_radius, max_radius, stats)
    kept = sift(centres(acc, threshold), min_d2, centre_capacity, stats)
    per = [radii(points, w, h, cx, cy, dp, threshold, min_radius, max_radius) for _, cx, cy in kept.tolist()]
    allc = np.concatenate(per).reshape(-1, 4) if per else np.empty((0, 4), f32)
    if stats is not None:
        stats["circles"] = stats.get("circles", 0) + len(allc)
        stats["two_radii"] = stats.get("two_radii", 0) + sum(len(c) >= 2 for c in per)
        stats["kept"] = stats.get("kept", 0) + len(kept)
    count = len(allc)
    k = count if capacity is None else min(count, int(capacity))
    return count, np.ascontiguousarray(allc[:k], f32)


def circles_batch(points, dx, dy, w, h, dp, min_dist, threshold, min_radius, max_radius, centre_capacity=MAX_CENTRES, capacity=None, stats=None):
    """(uint32 counts [n], [circles per frame]) of per-frame point lists and planes [n, h, w]."""
    res = [circles_of(p, gx, gy, w, h, dp, min_dist, threshold, min_radius, max_radius, centre_capacity, capacity, stats) for p, gx, gy in zip(points, dx, dy)]
    return np.array([c for c, _ in res], np.uint32), [s for _, s in res]


def draw(dx, dy, w, h, cx, cy, radius, strength=1000, steps=None):
    """The perimeter pixels of a circle as points int32 (k, 2), in the order of the angle and without repeats; their gradients,
    radial with the given length, are written into the planes dx, dy [h, w]."""
    steps = steps or max(8, int(8 * radius))
    pts, seen = [], set()
    for k in range(steps):
        a = 2 * math.pi * k / steps
        x, y = int(round(cx + radius * math.cos(a))), int(round(cy + radius * math.sin(a)))
        if 0 <= x < w and 0 <= y < h and (x, y) not in seen:
            seen.add((x, y))
            pts.append((x, y))
            dx[y, x], dy[y, x] = int(round(strength * math.cos(a))), int(round(strength * math.sin(a)))
    return np.array(pts, np.int32).reshape(-1, 2)
