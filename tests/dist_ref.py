"""hc_distance_transform_device restated in numpy (include/hipcanny.h states the rule): the exact squared Euclidean distance of
every pixel to the nearest feature pixel, its float32 root, and the index y' * W + x' of that pixel, ties to the smallest x', then
the smallest y'.

Two independent forms, and a third, `vectorised`, as exact as they are and fast on dense maps (tests/device_op_sequences.py):

* brute_force: all feature pixels sorted by (x', y'), the squared distances of a chunk of pixels to every one of them, argmin
  (numpy's takes the first minimum: the smallest (x', y') in that order).  Nothing of the kernels' structure is in it.
* separable: the two passes of dist.hip, in plain loops -- per column the vertical offset to the nearest feature pixel, a tie going
  to the one above; per pixel the outward search x - d, x + d that runs while d^2 <= best, the left side replacing on <=, the right
  side on <.  tests/test_dist_ref_cpu.py holds the two against each other and the distances against scipy.

A plain helper module (no fixtures)."""
import numpy as np

TO_NONZERO, TO_ZERO = 0, 1
NONE = 2147483647   # HC_DT_NONE


def features(m, target=TO_NONZERO):
    m = np.asarray(m)
    return (m != 0) if target == TO_NONZERO else (m == 0)


def brute_force(m, target=TO_NONZERO, budget=1 << 22):
    """(d2 int32 [H, W], nearest int32 [H, W]) of one map; `budget`: pixel x feature pairs held at a time."""
    feat = features(m, target)
    h, w = feat.shape
    ys, xs = np.nonzero(feat)
    if len(xs) == 0:
        return np.full((h, w), NONE, np.int32), np.full((h, w), -1, np.int32)
    order = np.lexsort((ys, xs))   # by x', then y'
    assert (w - 1) ** 2 + (h - 1) ** 2 < NONE and w * h < NONE   # the entry's own limits: everything below fits int32
    xs, ys = xs[order].astype(np.int32), ys[order].astype(np.int32)
    d2 = np.empty(h * w, np.int32)
    near = np.empty(h * w, np.int32)
    step = max(1, budget // len(xs))
    for p0 in range(0, h * w, step):
        p = np.arange(p0, min(p0 + step, h * w), dtype=np.int32)
        d = (p[:, None] % w - xs[None, :]) ** 2 + (p[:, None] // w - ys[None, :]) ** 2
        k = np.argmin(d, axis=1)
        d2[p] = d[np.arange(len(p)), k]
        near[p] = ys[k] * w + xs[k]
    return d2.reshape(h, w), near.reshape(h, w)


def column_pass(feat):
    """dy = y' - y of the nearest feature pixel of the column, a tie to the one above; None where the column has none."""
    h, w = feat.shape
    dy = [[None] * w for _ in range(h)]
    for x in range(w):
        last = None
        for y in range(h):
            if feat[y, x]:
                last = y
            if last is not None:
                dy[y][x] = last - y
        nxt = None
        for y in range(h - 1, -1, -1):
            if feat[y, x]:
                nxt = y
            elif nxt is not None and (dy[y][x] is None or nxt - y < -dy[y][x]):
                dy[y][x] = nxt - y
    return dy


def separable(m, target=TO_NONZERO):
    """The same pair by the kernels' two passes (plain loops: small frames only)."""
    feat = features(m, target)
    h, w = feat.shape
    dy = column_pass(feat)
    d2 = np.full((h, w), NONE, np.int32)
    near = np.full((h, w), -1, np.int32)
    if not feat.any():
        return d2, near
    for y in range(h):
        row = dy[y]
        for x in range(w):
            best, bx = (row[x] ** 2, x) if row[x] is not None else (NONE, x)
            d = 1
            while d * d <= best and (d <= x or x + d < w):
                if d <= x and row[x - d] is not None and d * d + row[x - d] ** 2 <= best:
                    best, bx = d * d + row[x - d] ** 2, x - d
                if x + d < w and row[x + d] is not None and d * d + row[x + d] ** 2 < best:
                    best, bx = d * d + row[x + d] ** 2, x + d
                d += 1
            d2[y, x] = best
            near[y, x] = (y + row[bx]) * w + bx
    return d2, near


def vectorised(m, target=TO_NONZERO, budget=1 << 22):
    """The same pair, exactly, in O(H W^2) numpy: per column the nearest feature pixel of every row (a tie to the one above, the
    smaller y'), then per pixel the minimum over all columns x' of (x - x')^2 + dy(y, x')^2, argmin taking the first, the smallest
    x'.  The nearest feature pixel overall lies in some column, and there it is that column's nearest: nothing is approximated.
    For the dense maps of the seeded chains, where brute_force is quadratic in the pixels; tests/test_dist_ref_cpu.py holds the
    two equal.  `budget`: pixel x column pairs held at a time."""
    feat = features(m, target)
    h, w = feat.shape
    if not feat.any():
        return np.full((h, w), NONE, np.int32), np.full((h, w), -1, np.int32)
    assert (w - 1) ** 2 + (h - 1) ** 2 < NONE and w * h < NONE
    far = 1 << 20                                         # (rows apart: above every H the squared diagonal admits)
    ys = np.arange(h, dtype=np.int64)[:, None]
    up = np.maximum.accumulate(np.where(feat, ys, -far), axis=0)                  # the last feature row at or above y
    down = np.minimum.accumulate(np.where(feat, ys, 2 * far)[::-1], axis=0)[::-1]   # the first at or below
    above = ys - up <= down - ys
    ny = np.where(above, up, down)                        # (a column without a feature pixel: -far, dy^2 beyond every distance)
    dy2 = (ny - ys) ** 2
    xs = np.arange(w, dtype=np.int64)
    dx2 = (xs[:, None] - xs[None, :]) ** 2                # [x, x']
    d2 = np.empty((h, w), np.int32)
    near = np.empty((h, w), np.int32)
    step = max(1, budget // (w * w))
    for y0 in range(0, h, step):
        y1 = min(y0 + step, h)
        cost = dx2[None, :, :] + dy2[y0:y1, None, :]      # [y, x, x']
        k = np.argmin(cost, axis=2)
        rows = np.arange(y0, y1)[:, None]
        d2[y0:y1] = np.take_along_axis(cost, k[:, :, None], axis=2)[:, :, 0]
        near[y0:y1] = ny[rows, k] * w + k
    return d2, near


def root_f32(d2):
    """HC_DT_F32 of squared distances: int32 -> float32 (round to nearest even), then the correctly rounded float32 square root;
    +inf where d2 == NONE."""
    d2 = np.asarray(d2, np.int32)
    return np.where(d2 == NONE, np.float32(np.inf), np.sqrt(d2.astype(np.float32))).astype(np.float32)


def distance_transform(maps, target=TO_NONZERO, form=brute_force):
    """(d2 int32 [n, H, W], nearest int32 [n, H, W]) of a batch, frame by frame, by brute force (or form=vectorised)."""
    pairs = [form(m, target) for m in maps]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
