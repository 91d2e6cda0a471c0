"""The restatement of hc_connected_components_device (include/hipcanny.h): numpy and a plain flood fill.

A pixel is foreground iff its byte is non-zero.  A component is a maximal set of foreground pixels connected through 4 (edge) or
8 (edge or corner) neighbours.  Its first pixel is the one with the smallest y * W + x; components are numbered 1, 2, ... in
ascending order of their first pixels, background is 0 -- the order a raster scan meets them in, so the fill below simply starts
a new component at every foreground pixel the scan reaches unnumbered.

Row k of the statistics is (left, top, width, height, area) of component k (row 0: the background), its centroid
(float64(sx) / float64(area), float64(sy) / float64(area)) with sx, sy the exact integer sums of x and y.  A background without
a pixel is five zeros and (0.0, 0.0)."""
import numpy as np

STAT_WORDS = 5
NEIGHBOURS = {4: ((0, -1), (0, 1), (-1, 0), (1, 0)),
              8: ((0, -1), (0, 1), (-1, 0), (1, 0), (-1, -1), (-1, 1), (1, -1), (1, 1))}


def label(m, connectivity=8):
    """(int32 labels [H, W], N = components + 1) of one map."""
    nb = NEIGHBOURS[connectivity]
    fg = np.asarray(m) != 0
    h, w = fg.shape
    lab = [[0] * w for _ in range(h)]   # (plain lists: the fill touches single elements)
    n = 0
    fgl = fg.tolist()
    for y0, x0 in zip(*(v.tolist() for v in np.nonzero(fg))):   # raster order
        if lab[y0][x0]:
            continue
        n += 1
        lab[y0][x0] = n
        stack = [(y0, x0)]
        while stack:
            y, x = stack.pop()
            for dy, dx in nb:
                yy, xx = y + dy, x + dx
                if 0 <= yy < h and 0 <= xx < w and fgl[yy][xx] and not lab[yy][xx]:
                    lab[yy][xx] = n
                    stack.append((yy, xx))
    return np.array(lab, np.int32).reshape(h, w), n + 1


def stats_of(lab, n):
    """(int32 [n, 5], float64 [n, 2]) of a label image with numbers 0 .. n - 1."""
    h, w = lab.shape
    st = np.zeros((n, STAT_WORDS), np.int32)
    cen = np.zeros((n, 2), np.float64)
    ys, xs = np.mgrid[0:h, 0:w]
    for k in range(n):
        sel = lab == k
        area = int(sel.sum())
        if area == 0:
            continue   # only the background of a full frame
        x, y = xs[sel], ys[sel]
        st[k] = (x.min(), y.min(), x.max() - x.min() + 1, y.max() - y.min() + 1, area)
        cen[k] = (np.float64(int(x.sum())) / np.float64(area), np.float64(int(y.sum())) / np.float64(area))
    return st, cen


def stats_fast(lab, n):
    """stats_of by sorting: the same values for maps with thousands of components."""
    h, w = lab.shape
    flat = lab.reshape(-1).astype(np.int64)
    ys, xs = np.divmod(np.arange(h * w, dtype=np.int64), w)
    order = np.argsort(flat, kind="stable")
    f, x, y = flat[order], xs[order], ys[order]
    st = np.zeros((n, STAT_WORDS), np.int32)
    cen = np.zeros((n, 2), np.float64)
    present, first = np.unique(f, return_index=True)
    area = np.diff(np.append(first, f.size))
    minx, maxx = np.minimum.reduceat(x, first), np.maximum.reduceat(x, first)
    miny, maxy = np.minimum.reduceat(y, first), np.maximum.reduceat(y, first)
    sx, sy = np.add.reduceat(x, first), np.add.reduceat(y, first)
    st[present] = np.stack([minx, miny, maxx - minx + 1, maxy - miny + 1, area], axis=1)
    cen[present] = np.stack([sx.astype(np.float64) / area.astype(np.float64), sy.astype(np.float64) / area.astype(np.float64)], axis=1)
    return st, cen


def _pixels_row(x, y):
    """(statistics row, centroid) of a set of pixels given by its coordinates: the sums are Python ints until the two divisions."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    area = int(x.size)
    if area == 0:
        return (0, 0, 0, 0, 0), (0.0, 0.0)
    left, top = int(x.min()), int(y.min())
    return (left, top, int(x.max()) - left + 1, int(y.max()) - top + 1, area), (np.float64(int(x.sum())) / np.float64(area), np.float64(int(y.sum())) / np.float64(area))


def checkerboard4(w, h):
    """(labels, N, statistics, centroids) of the map (x + y) % 2 == 0 at connectivity 4, in closed form, no fill: no two foreground
    pixels share an edge, so each is a component of its own, numbered in raster order -- row k is (x, y, 1, 1, 1) with the
    centroid (x, y); row 0 is the other colour of the board."""
    yy, xx = np.mgrid[0:h, 0:w]
    fg = (xx + yy) % 2 == 0
    n = int(fg.sum()) + 1
    labels = np.zeros((h, w), np.int32)
    labels[fg] = np.arange(1, n, dtype=np.int32)
    st = np.ones((n, STAT_WORDS), np.int32)
    cen = np.zeros((n, 2), np.float64)
    st[1:, 0], st[1:, 1] = xx[fg], yy[fg]
    cen[1:, 0], cen[1:, 1] = xx[fg], yy[fg]
    st[0], cen[0] = _pixels_row(xx[~fg], yy[~fg])
    return labels, n, st, cen


def columns(w, h, x1):
    """(labels, N, statistics, centroids) of the map whose columns [0, x1) are foreground, at either connectivity, in closed form:
    x1 = w is the full frame, x1 = 0 the empty one.  One rectangle and the rectangle behind it; a rectangle of the columns
    [a, b) has the sums (b - a) * h * (a + b - 1) / 2 of x and (b - a) * h * (h - 1) / 2 of y, exact as Python ints."""
    def rect(a, b):
        area = (b - a) * h
        if area == 0:
            return (0, 0, 0, 0, 0), (0.0, 0.0)
        sx, sy = (b - a) * h * (a + b - 1) // 2, (b - a) * h * (h - 1) // 2
        return (a, 0, b - a, h, area), (np.float64(sx) / np.float64(area), np.float64(sy) / np.float64(area))
    n = 2 if x1 > 0 else 1
    labels = np.zeros((h, w), np.int32)
    labels[:, :x1] = 1
    rows = [rect(x1, w), rect(0, x1)][:n]
    return labels, n, np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.float64)


def connected_components(maps, connectivity=8, capacity=None):
    """maps (n, H, W) -> (int32 labels (n, H, W), uint32 counts (n), [int32 (min(N, capacity), 5)], [float64 (min(N, capacity), 2)]);
    capacity None: every row."""
    maps = np.asarray(maps)
    labels = np.zeros(maps.shape, np.int32)
    counts = np.zeros(maps.shape[0], np.uint32)
    stats, cents = [], []
    for f, m in enumerate(maps):
        labels[f], n = label(m, connectivity)
        counts[f] = n
        st, cen = stats_fast(labels[f], n)
        k = n if capacity is None else min(n, capacity)
        stats.append(st[:k])
        cents.append(cen[:k])
    return labels, counts, stats, cents
