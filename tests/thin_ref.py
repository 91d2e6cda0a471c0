"""hc_thinning_device restated in numpy: the Zhang-Suen and Guo-Hall thinning of binary maps as include/hipcanny.h states them.

Neighbours of P1 = (y, x), clockwise from north: P2 (y-1, x), P3 (y-1, x+1), P4 (y, x+1), P5 (y+1, x+1), P6 (y+1, x), P7 (y+1, x-1),
P8 (y, x-1), P9 (y-1, x-1); a position outside the frame is background, and every pixel of the frame is a candidate (the textbook
rule).  All decisions of a sub-iteration are taken on the map as it was when the sub-iteration began.

`thin` is the restatement the GPU tests compare with (eight shifted views of the zero-padded map).  `thin_naive` is a second,
deliberately naive one -- a Python loop over pixels with the neighbour list written out -- used on tiny frames only, to guard the
first (tests/test_thin_ref_cpu.py)."""
import numpy as np

ZHANGSUEN, GUOHALL = 0, 1
METHODS = (ZHANGSUEN, GUOHALL)
METHOD_NAMES = {"zhangsuen": ZHANGSUEN, "guohall": GUOHALL}
MAX_ITERATIONS = 1024


def neighbours(m):
    """(P2, .., P9) of a bool map [H, W] as bool maps of the same shape."""
    h, w = m.shape
    p = np.pad(m, 1)

    def s(dy, dx):
        return p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    return s(-1, 0), s(-1, 1), s(0, 1), s(1, 1), s(1, 0), s(1, -1), s(0, -1), s(-1, -1)


def removed_by(m, method, s):
    """The pixels sub-iteration s (0 or 1) removes from the bool map m."""
    p2, p3, p4, p5, p6, p7, p8, p9 = neighbours(m)
    if method == ZHANGSUEN:
        ring = [p2, p3, p4, p5, p6, p7, p8, p9, p2]
        b = sum(q.astype(np.int32) for q in ring[:8])
        a = sum((~ring[i] & ring[i + 1]).astype(np.int32) for i in range(8))
        cond = (~(p2 & p4 & p6) & ~(p4 & p6 & p8)) if s == 0 else (~(p2 & p4 & p8) & ~(p2 & p6 & p8))
        return m & (b >= 2) & (b <= 6) & (a == 1) & cond
    if method != GUOHALL:
        raise ValueError(f"method {method}")
    i32 = np.int32
    c = (~p2 & (p3 | p4)).astype(i32) + (~p4 & (p5 | p6)).astype(i32) + (~p6 & (p7 | p8)).astype(i32) + (~p8 & (p9 | p2)).astype(i32)
    n1 = (p9 | p2).astype(i32) + (p3 | p4).astype(i32) + (p5 | p6).astype(i32) + (p7 | p8).astype(i32)
    n2 = (p2 | p3).astype(i32) + (p4 | p5).astype(i32) + (p6 | p7).astype(i32) + (p8 | p9).astype(i32)
    n = np.minimum(n1, n2)
    mm = ((p6 | p7 | ~p9) & p8) if s == 0 else ((p2 | p3 | ~p5) & p4)
    return m & (c == 1) & (n >= 2) & (n <= 3) & ~mm


def iterate(m, method):
    """One iteration (sub-iteration 0, then 1) of a bool map: (the new map, the number of pixels removed)."""
    r = 0
    for s in (0, 1):
        gone = removed_by(m, method, s)
        r += int(gone.sum())
        m = m & ~gone
    return m, r


def thin(map_, method, max_iterations):
    """One frame [H, W] (foreground: non-zero) -> (uint8 0 / 255 map, iterations that removed a pixel, converged 0 / 1): the map
    after min(K - 1, max_iterations) iterations, K the first iteration within max_iterations that removes nothing."""
    if not 1 <= int(max_iterations) <= MAX_ITERATIONS:
        raise ValueError("max_iterations outside 1..1024")
    m = np.asarray(map_) != 0
    assert m.ndim == 2
    for k in range(int(max_iterations)):
        nxt, r = iterate(m, method)
        if r == 0:
            return (m * np.uint8(255)).astype(np.uint8), k, 1
        m = nxt
    return (m * np.uint8(255)).astype(np.uint8), int(max_iterations), 0


def thin_batch(maps, method, max_iterations):
    """[n, H, W] -> (uint8 maps [n, H, W], uint32 status [n, 2] = (iterations, converged))."""
    res = [thin(f, method, max_iterations) for f in maps]
    return np.stack([r[0] for r in res]), np.array([[r[1], r[2]] for r in res], np.uint32).reshape(len(res), 2)


# ---- the naive restatement ---------------------------------------------------------------------------------------------------
def removed_by_naive(m, method, s):
    h, w = len(m), len(m[0])

    def at(y, x):
        return 1 if 0 <= y < h and 0 <= x < w and m[y][x] else 0
    gone = []
    for y in range(h):
        for x in range(w):
            if not m[y][x]:
                continue
            p2, p3, p4, p5 = at(y - 1, x), at(y - 1, x + 1), at(y, x + 1), at(y + 1, x + 1)
            p6, p7, p8, p9 = at(y + 1, x), at(y + 1, x - 1), at(y, x - 1), at(y - 1, x - 1)
            if method == ZHANGSUEN:
                ring = [p2, p3, p4, p5, p6, p7, p8, p9, p2]
                b = sum(ring[:8])
                a = sum(1 for i in range(8) if ring[i] == 0 and ring[i + 1] == 1)
                ok = 2 <= b <= 6 and a == 1
                if s == 0:
                    ok = ok and p2 * p4 * p6 == 0 and p4 * p6 * p8 == 0
                else:
                    ok = ok and p2 * p4 * p8 == 0 and p2 * p6 * p8 == 0
            else:
                c = ((1 - p2) & (p3 | p4)) + ((1 - p4) & (p5 | p6)) + ((1 - p6) & (p7 | p8)) + ((1 - p8) & (p9 | p2))
                n1 = (p9 | p2) + (p3 | p4) + (p5 | p6) + (p7 | p8)
                n2 = (p2 | p3) + (p4 | p5) + (p6 | p7) + (p8 | p9)
                n = min(n1, n2)
                mm = ((p6 | p7 | (1 - p9)) & p8) if s == 0 else ((p2 | p3 | (1 - p5)) & p4)
                ok = c == 1 and 2 <= n <= 3 and mm == 0
            if ok:
                gone.append((y, x))
    return gone


def iterate_naive(m, method):
    """One iteration of a list-of-lists 0 / 1 map: (the new map, the number of pixels removed)."""
    m = [list(row) for row in m]
    r = 0
    for s in (0, 1):
        gone = removed_by_naive(m, method, s)
        for y, x in gone:
            m[y][x] = 0
        r += len(gone)
    return m, r


# ---- test content --------------------------------------------------------------------------------------------------------------
def blobs(h, w, seed, sigma=2.0, cut=0.5):
    """Seeded blob frames: scipy.ndimage.gaussian_filter of uniform noise, cut at `cut`."""
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    return ((ndimage.gaussian_filter(rng.random((h, w)), sigma) > cut) * 255).astype(np.uint8)
