"""The frames, points and parameters of the optical-flow cases that tests/test_gpu_flow.py runs on the device and whose
preconditions tests/test_flow_ref_cpu.py asserts on the reference alone (tests/flow_ref.py): what each case is FOR -- a window
class, a sum beyond 32 bits, 64 iterations, a tracked point on a plane smaller than the window -- is a property of the reference's
run on this content, found by a search on the CPU and checked there, so that the device test compares words that matter.  Pure
numpy; no GPU."""
import numpy as np

from cudacam_amd import synth
import flow_ref as R

WINDOWS = tuple(range(5, 32, 2))   # every window the contract allows
ROUND_CLASSES = (1, 2, 4, 7, 10, 16)


def flow_rounds(win):
    """canny_params.h restated: rounds of 64 window pixels, and the compiled kernel (class) that serves them"""
    return (win * win + 63) // 64


def flow_round_class(win):
    return min(c for c in ROUND_CLASSES if c >= flow_rounds(win))


def idle_rounds(win):
    """rounds of the window's kernel in which no lane has a pixel (13: 1 of 4; 17, 19: 2 and 1 of 7; 23: 1 of 10; 27, 29: 4 and 2 of 16)"""
    return flow_round_class(win) - flow_rounds(win)


def pair(w, h, seed, shift=(1, 2)):
    a = synth.natural(w, h, seed)
    return a, np.ascontiguousarray(np.roll(a, shift, (0, 1)))


def points(w, h, win, rng):
    """integer, half and arbitrary sub-pixel positions; within win of each border and each corner; exactly out of frame by the rule
    and just inside it; NaN; far away"""
    hw = (win - 1) * 0.5
    pts = [(w // 2, h // 2), (w // 2 + 0.5, h // 2 - 0.5), (w // 3 + 0.5, h // 3)]
    pts += [tuple(rng.uniform([4, 4], [w - 4, h - 4])) for _ in range(5)]
    pts += [(1.25, h / 2), (w - 1.5, h / 2), (w / 2, 0.75), (w / 2, h - 1.0), (0, 0), (w - 1, 0), (0.5, h - 1), (w - 1.25, h - 1.5), (win - 1.5, win - 2.25)]
    # the rule is on floor(p - hw): out at floor < -win and at floor >= w
    pts += [(hw - win - 0.25, h / 2), (hw - win, h / 2), (w + hw, h / 2), (w + hw - 0.25, h / 2), (w / 2, hw - win - 0.5), (w / 2, h + hw - 0.5), (w / 2, h + hw)]
    pts += [(np.nan, 5.0), (5.0, np.nan), (1e12, 3.0), (-3e9, 3.0), (np.inf, 1.0)]
    return np.float32(pts)


def infos(prev, nxt, level, pts, start, win, iters, eps, thr, use_initial):
    """flow_ref.lk_point's (status, info) of every point of one frame"""
    out = []
    for p, q in zip(pts, start):
        _, st, _, info = R.lk_point(prev, nxt, level, p, q, win, iters, eps, thr, use_initial)
        out.append((st, info))
    return out


def everywhere(w, h, win, seed):
    """The frame pair and points of test_flow_points_everywhere: a seeded natural frame and its copy rolled by (1, 2), both with a
    flat rectangle (points there are lost by the eigenvalue rule), and the points of `points` plus one inside the rectangle."""
    a, b = pair(w, h, seed)
    a[h // 2 - 3:h // 2 + 8, 4:15] = 77
    b[h // 2 - 3:h // 2 + 8, 4:15] = 77
    rng = np.random.default_rng(win * 100 + w)
    pts = np.concatenate([points(w, h, win, rng), np.float32([[7.5, h // 2 + 1.25]])])
    return a, b, pts, rng


# ---- every window on one small frame ---------------------------------------------------------------------------------------------
WIN_W, WIN_H = 48, 40
WIN_RUNS = ((30, 0.01, 0, True), (30, 0.01, 1, False), (2, 0.0, 0, False), (30, 0.0, 1, True))   # iterations, epsilon, use_initial, err


def window_case(win):
    """48 x 40 -- narrower than the reach of the largest windows from any point --: (prev, next, points, starts), a start per run"""
    a, b, pts, rng = everywhere(WIN_W, WIN_H, win, 300 + win)
    starts = [(pts + rng.uniform(-1.5, 1.5, pts.shape).astype(np.float32)) for _ in WIN_RUNS]
    return a, b, pts, starts


# ---- planes smaller than the window --------------------------------------------------------------------------------------------
TINY_SHAPES = ((1, 1), (1, 9), (9, 1), (6, 5))
TINY_WINDOWS = (5, 31)
TINY_SEED = 3   # (the seed of the 6 x 5 content: the reference tracks points of it at both windows -- test_flow_ref_cpu.py)


def tiny_case(w, h, win):
    """Seeded random bytes (1 x 1, 1 x 9, 9 x 1: no gradient in at least one direction, every point is lost) or, 6 x 5, a seeded
    smooth blob and its copy moved by half a pixel: (prev, next, points)"""
    rng = np.random.default_rng(TINY_SEED * 1000 + w * 10 + h)
    if (w, h) == (6, 5):
        y, x = np.mgrid[0:h, 0:w].astype(np.float64)
        blob = lambda cx, cy: np.clip(np.rint(30 + 200 * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / 4.0)), 0, 255).astype(np.uint8)
        a, b = blob(2.5, 2.0), blob(3.0, 2.25)
    else:
        a = rng.integers(0, 256, (h, w), dtype=np.uint8)
        b = rng.integers(0, 256, (h, w), dtype=np.uint8)
    hw = (win - 1) * 0.5
    pts = [(0, 0), (w - 1, h - 1), ((w - 1) / 2, (h - 1) / 2), (w / 2 + 0.25, h / 2 - 0.25), (w - 0.5, 0.5), (-1.5, 2.0), (w + 1.0, h + 0.75)]
    pts += [(hw - win, 0.0), (hw - win - 0.25, 0.0), (w + hw - 0.25, 0.0), (w + hw, 0.0), (0.0, h + hw - 0.25), (0.0, h + hw)]
    pts += [tuple(rng.uniform([-2, -2], [w + 2, h + 2])) for _ in range(5)]
    return a, b, np.float32(pts)


# ---- level 15 ----------------------------------------------------------------------------------------------------------------------
TOP_LEVEL, TOP_W, TOP_H, TOP_WIN = 15, 12, 10, 5


def top_level_case():
    """A 12 x 10 plane as level 15 of its frame: (prev, next, prev_pts in level-0 units, start)"""
    a, b = pair(TOP_W, TOP_H, 4, (0, 1))
    rng = np.random.default_rng(15)
    plane = np.concatenate([rng.uniform([1, 1], [TOP_W - 1, TOP_H - 1], (10, 2)), [[0, 0], [TOP_W - 1, TOP_H - 1], [-4.0, 3.0], [TOP_W + 2.0, 3.0], [3.0, -4.5], [5.5, TOP_H + 2.0],
                                                                                   [np.nan, 1.0]]])
    pts = (plane * 32768.0).astype(np.float32)
    start = (pts + rng.uniform(-0.75, 0.75, pts.shape).astype(np.float32) * np.float32(32768.0)).astype(np.float32)
    return a, b, pts, start


# ---- 64 iterations ---------------------------------------------------------------------------------------------------------------
LONG_W, LONG_H, LONG_WIN = 48, 40, 9


def long_case():
    """(prev, next, points) on which the reference, with epsilon 0, runs all 64 iterations for some points: see test_flow_ref_cpu.py"""
    a = synth.natural(LONG_W, LONG_H, 2)
    b = np.random.default_rng(2).integers(0, 256, (LONG_H, LONG_W), dtype=np.uint8)
    rng = np.random.default_rng(64)
    return a, b, rng.uniform([6, 6], [LONG_W - 6, LONG_H - 6], (24, 2)).astype(np.float32)


# ---- sums beyond 32 bits -----------------------------------------------------------------------------------------------------------
BIG_W, BIG_H = 64, 48
BIG_WINDOWS = (25, 27, 29, 31)
BIG_SEED = 1
BIG_ROLLS = ((1, 1), (-1, -1))


def big_sum_case(roll):
    """Seeded 2 x 2 blocks of 0 / 255 and their copy rolled by `roll`: window sums of gradient squares reach 2^32, those of
    difference times gradient +-2^31.  (prev, next, points)"""
    g = np.random.default_rng(BIG_SEED).integers(0, 2, (BIG_H // 2, BIG_W // 2))
    a = (np.kron(g, np.ones((2, 2), dtype=np.int64)) * 255).astype(np.uint8)
    b = np.ascontiguousarray(np.roll(a, roll, (0, 1)))
    cx, cy = BIG_W // 2, BIG_H // 2
    pts = np.float32([(cx, cy), (cx + 0.5, cy - 0.25), (cx - 6, cy + 3), (cx + 7.25, cy - 4.5), (20, 20), (44, 28), (cx, 16.5), (18.75, cy)])
    return a, b, pts


STRIPE_WINDOWS = (29, 31)
STRIPE_ROLLS = ((0, 1), (0, -1))


def stripe_sum_case(roll):
    """Beyond the blocks: the wave sum is made of four sums of 16 lanes each, and on the blocks none of those leaves int32 -- only
    their total does.  Vertical stripes 2 pixels wide have |gx| = 4080 at every pixel (the largest there is); a tenth of the 2 x 2
    blocks, seeded, hold 0 / 255 at random instead and give the gradient in y a point needs to be tracked.  A sum at or beyond
    +-2^33 has a sixteen-lane part at or beyond +-2^31.  `next` is `prev` rolled by one column.  (prev, next, points)"""
    rng = np.random.default_rng(0)
    a = np.tile(((np.arange(BIG_W) // 2) % 2 * 255).astype(np.uint8), (BIG_H, 1))
    g = np.kron(rng.integers(0, 2, (BIG_H // 2, BIG_W // 2)), np.ones((2, 2), dtype=np.int64)) * 255
    m = np.kron(rng.random((BIG_H // 2, BIG_W // 2)) < 0.1, np.ones((2, 2), dtype=bool))
    a = np.where(m, g, a).astype(np.uint8)
    b = np.ascontiguousarray(np.roll(a, roll, (0, 1)))
    return a, b, np.float32([(32, 24), (32.5, 23.75), (26, 27), (39.25, 19.5)])


# ---- a pyramid that stops early------------------------------------------------------------------------------------------------
STOP_W, STOP_H, STOP_LEVELS, STOP_WIN = 20, 9, 5, 9


def stop_case():
    """20 x 9 with levels = 5: 10 x 5 and 5 x 3 follow, and a fourth plane would have a side below 3.  (prev, next, points, counts)"""
    frames = [pair(STOP_W, STOP_H, 40 + f, (0, 1)) for f in range(2)]
    a, b = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    pts = np.random.default_rng(9).uniform([1, 1], [STOP_W - 1, STOP_H - 1], (2, 10, 2)).astype(np.float32)
    return a, b, pts, [10, 7]


# ---- an eight-lane sum beyond 32 bits ----------------------------------------------------------------------------------------
ROW_WIN = 31
ROW_ROLLS = ((1, 0), (-1, 0))


def row_sum_case(roll):
    """Inside the wave sum, the only values that travel between lanes as two halves AND can leave int32 are eight-lane sums of
    diff * g (8 lanes x 16 rounds x 8160 x 4080 = 4.26e9; of squares, 2.13e9 < 2^31).  Lane l owns the window pixels t = l + 64 r at
    (t % win, t / win): at window 31 the pixels of lanes 0 .. 7 lie in the even window rows, all but five.  Horizontal stripes 2
    pixels high have |gy| = 4080 everywhere, and against their copy rolled by one row diff * gy is +-8160 * 4080 in every second
    row, one sign, zero between -- with the right row parity that is nearly every pixel of those eight lanes.  A tenth of the 2 x 2
    blocks hold seeded 0 / 255 for the gradient in x a tracked point needs.  (prev, next, points)"""
    rng = np.random.default_rng(0)
    a = np.tile(((np.arange(BIG_H) // 2) % 2 * 255).astype(np.uint8)[:, None], (1, BIG_W))
    g = np.kron(rng.integers(0, 2, (BIG_H // 2, BIG_W // 2)), np.ones((2, 2), dtype=np.int64)) * 255
    m = np.kron(rng.random((BIG_H // 2, BIG_W // 2)) < 0.1, np.ones((2, 2), dtype=bool))
    a = np.where(m, g, a).astype(np.uint8)
    b = np.ascontiguousarray(np.roll(a, roll, (0, 1)))
    return a, b, np.float32([(32, 24), (32, 25), (31, 23), (33, 22)])


def first_products(prev, nxt, pt, win):
    """(diff * gx, diff * gy) of every window pixel [win, win] in the first iteration from pt itself, level 0: what the lanes add"""
    jj, ii = np.mgrid[0:win, 0:win]
    hw = R.F(R.F(win - 1) * R.F(0.5))
    ix, iy, wts = R._weights((R.F(pt[0] - hw), R.F(pt[1] - hw)))
    I = (R._interp(lambda x, y: R._pix(prev, x, y), ix, iy, wts, ii, jj) + 256) >> 9
    J = (R._interp(lambda x, y: R._pix(nxt, x, y), ix, iy, wts, ii, jj) + 256) >> 9
    gx = (R._interp(lambda x, y: R._scharr(prev, x, y)[0], ix, iy, wts, ii, jj) + 8192) >> 14
    gy = (R._interp(lambda x, y: R._scharr(prev, x, y)[1], ix, iy, wts, ii, jj) + 8192) >> 14
    return (J - I) * gx, (J - I) * gy


def lane_group_sums(products, lanes):
    """the sums over groups of `lanes` consecutive lanes of a wave, pixel t = j * win + i with lane t % 64 (flow.hip)"""
    lane = np.arange(products.size) % 64
    flat = products.reshape(-1)
    return [int(flat[lane // lanes == g].sum()) for g in range(64 // lanes)]
