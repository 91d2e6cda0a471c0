"""Tri-state maps (0 / 128 / 255) aimed at how k_hyst (cudacam_amd/csrc/hyst.hip) propagates, pure numpy.

k_hyst is not a pixel-per-iteration hysteresis.  A wave fills a whole candidate run of a row in one step (row_fill: a carry
look-ahead over lane ballots), settles everything that stays inside its own rows by itself, hands a boundary row to the next
wave once per ROUND of the tile loop and a tile boundary row / column to the next tile once per LAUNCH.  So what costs it
time is not the length of a path but how often the path changes wave (rounds, capped at HYST_ROUND_CAP per launch) and tile
(launches).  synth.thresh_map_serpentine calls itself the worst case for tile-iterated hysteresis; for this kernel it is
close to the best one -- every run is one carry, every connector one step of a downward sweep, a tile boundary is crossed
once.  The worst case is its transpose, `vertical_serpentine`: every column crosses every wave boundary.

Every generator returns read-only arrays, and with the map what a CPU test needs to show that the map is not vacuous: the
path in order, or the result the case itself states (tests/test_hyst_maps_cpu.py holds oracle.hysteresis against it)."""
import numpy as np

PANEL_COLS = 2048   # columns of a column panel of k_hyst: 64 lanes x 32 bits


def _frozen(a):
    a.setflags(write=False)
    return a


def _map_of(path, w, h):
    t = np.zeros((h, w), np.uint8)
    p = np.asarray(path)
    t[p[:, 0], p[:, 1]] = 128
    return t


# ---- paths -------------------------------------------------------------------------------------------------------------------
def vertical_serpentine(w, h, r0, r1, ncols):
    """(map, path): a 1-px candidate path down column 1, up column 3, down column 5, ... -- `ncols` columns over the rows r0 ..
    r1 - 1, single-pixel connectors in the even columns alternating between the band's last and first row -- with one strong
    pixel at (r0, 1).  path: its pixels (row, col) in order from the seed."""
    assert 0 <= r0 < r1 <= h and r1 - r0 >= 3 and ncols >= 1 and 2 * ncols - 1 < w
    path = []
    for k in range(ncols):
        x = 2 * k + 1
        rows = range(r0, r1) if k % 2 == 0 else range(r1 - 1, r0 - 1, -1)
        path.extend((y, x) for y in rows)
        if k + 1 < ncols:
            path.append((r1 - 1 if k % 2 == 0 else r0, x + 1))
    t = _map_of(path, w, h)
    t[r0, 1] = 255
    return _frozen(t), tuple(path)


def _crossings(path, tile_rows, waves):
    rows = np.asarray(path)[:, 0]
    tile = tile_rows * waves
    bt, wv = rows // tile, (rows % tile) // tile_rows
    tiles = bt[1:] != bt[:-1]
    return int(np.count_nonzero(~tiles & (wv[1:] != wv[:-1]))), int(np.count_nonzero(tiles))


def wave_crossings(path, tile_rows, waves):
    """Steps of `path` whose two pixels lie in different waves' rows of the same row tile (a workgroup tile = `waves` waves x
    `tile_rows` rows).  For a 1-px path from one seed: the sequential rounds of k_hyst's tile loop the path needs."""
    return _crossings(path, tile_rows, waves)[0]


def tile_crossings(path, tile_rows, waves):
    """Steps of `path` from one row tile to another: the sequential launches it needs beyond the first."""
    return _crossings(path, tile_rows, waves)[1]


def spiral(w, h, pitch, seed_at):
    """(map, path): a rectangular spiral, 1 px wide, from the frame's corner (0, 0) inwards, its arms `pitch` pixels apart
    (pitch >= 3), with one strong pixel at its outer end (seed_at "outer") or its inner end ("centre")."""
    assert pitch >= 3 and seed_at in ("outer", "centre")
    top, right, bottom, left = 0, w - 1, h - 1, 0   # the free rectangle: an arm ends at its side
    y, x, path = 0, 0, [(0, 0)]
    for d in range(2 * (w + h)):
        k = d % 4   # to the right, down, to the left, up
        n = (right - x, bottom - y, x - left, y - top)[k]
        if n < pitch:   # (every arm is at least `pitch` long, so the arms beside it are that far apart)
            break
        dy, dx = ((0, 1), (1, 0), (0, -1), (-1, 0))[k]
        for _ in range(n):
            y, x = y + dy, x + dx
            path.append((y, x))
        # the arm just walked takes `pitch` rows / columns off the free rectangle
        if k == 0: top += pitch
        elif k == 1: right -= pitch
        elif k == 2: bottom -= pitch
        else: left += pitch
    t = _map_of(path, w, h)
    assert np.count_nonzero(t) == len(path), "the spiral runs over itself"
    sy, sx = path[0] if seed_at == "outer" else path[-1]
    t[sy, sx] = 255
    return _frozen(t), tuple(path if seed_at == "outer" else path[::-1])


# The serpentines of tests/test_gpu_hyst_content.py: name -> (w, h, r0, r1, ncols, (tile_rows, waves) the case runs with;
# None: the shape a single frame gets by default).  tests/test_hyst_maps_cpu.py holds their wave crossings against
# HYST_ROUND_CAP: the "short" ones stay below half the cap, the "long" ones need more than 1.5 times the cap.
# (short_seam: 1056 columns reach over the panel seam at column 2048; at seven wave boundaries per column they would need 7.4 k
# rounds, so its band is the rows of the first two waves only: one wave boundary per column.)
# The widths: 2048 columns fill every lane of a panel, but such a frame has TWO panels, the second without a column (`panels`
# below), and k_hyst_loop takes one-panel frames only.  1984 is the widest one-panel frame: its cases reach k_hyst_loop and the
# kernels compiled without the panel code, the 2048 ones the kernels with it.
SERPENTINES = {
    "short": (2048, 128, 1, 127, 256, None),
    "short_1984": (1984, 128, 1, 127, 256, None),
    "short_seam": (2112, 128, 1, 31, 1056, None),
    "long": (2048, 128, 1, 127, 1023, None),
    "long_1984": (1984, 128, 1, 127, 992, None),
    "long_3216": (2048, 512, 1, 511, 1023, (32, 16)),
    "long_3216_1984": (1984, 512, 1, 511, 992, (32, 16)),
}
ONE_PANEL_MAX_W = 1984


def panels(w):
    """Column panels of a frame w wide (plane_row_dwords, cudacam_amd/csrc/host_plan.h: a bit-plane row holds W bits, and 31
    bytes for each 248-column strip of the front kernels, in 64, 128 or 256 dwords)."""
    need = max((w + 31) // 32, ((w + 247) // 248 * 31 + 3) // 4)
    assert need <= 256
    return 1 if need <= 64 else 2 if need <= 128 else 4


# ---- rows --------------------------------------------------------------------------------------------------------------------
ROW_FRAME_H = 64    # height of a frame of row_cases: four waves of the default shape, case rows 1, 4, ..., 61 (16: a wave's first)
_ENDS = (0, 1, 30, 31, 32, 33, 63, 64, 65, 1023, 1024, 2015, 2016, 2046, 2047)
_GAPS = (31, 32, 63, 64, 1023, 1024)


def row_cases(w):
    """(maps, expected, cases) for row_fill's carries and row_dilate's lane steps at width w.

    maps, expected: u8 (frames, ROW_FRAME_H, w), the tri-state maps and the result every case states for itself.  cases: a
    tuple of (frame, row, kind), one per case.  A case owns map rows row - 1 .. row + 1 (row = 1, 4, 7, ...), of which the last
    or the two outer ones stay empty, so cases do not touch:
    - for every start <= end of the endpoint set (lane and panel ends; module constants), the candidate run [start, end] with
      its seed at the start, the end, the middle -- the whole run is promoted -- and, where that column exists, with no seed of
      its own below a lone strong pixel at (row - 1, start - 1) / (row - 1, end + 1);
    - for every gap g, the runs [0, g - 1] and [g + 1, w - 1] with the seed at column 0 (only the left run is promoted) and at
      column w - 1 (only the right one);
    - no wrap: a strong pixel at (row, w - 1) with candidates at (row, 0) and (row + 1, 0), and the mirror image: nothing is
      promoted."""
    # (the last two columns at every width, not only beyond one panel: a run that ends where the row's zero padding begins)
    ends = sorted({e for e in _ENDS + (w - 2, w - 1) + ((PANEL_COLS, PANEL_COLS + 1) if w > PANEL_COLS else ()) if 0 <= e < w})
    gaps = [g for g in _GAPS + ((PANEL_COLS - 1, PANEL_COLS) if w > PANEL_COLS else ()) if 1 <= g and g + 1 <= w - 1]
    rows = []   # per case: (kind, {dy: [(c0, c1, value), ...]}, {dy: [(c0, c1), ...] promoted})
    for i, a in enumerate(ends):
        for b in ends[i:]:
            for name, s in (("start", a), ("end", b), ("middle", (a + b) // 2)):
                rows.append((f"run [{a}, {b}] seed at its {name} {s}", {0: [(a, b, 128), (s, s, 255)]}, {0: [(a, b)]}))
            for name, s in (("start - 1", a - 1), ("end + 1", b + 1)):
                if 0 <= s < w:
                    rows.append((f"run [{a}, {b}] below a strong pixel at {name} {s}", {-1: [(s, s, 255)], 0: [(a, b, 128)]}, {-1: [(s, s)], 0: [(a, b)]}))
    for g in gaps:
        both = [(0, g - 1, 128), (g + 1, w - 1, 128)]
        rows.append((f"runs [0, {g - 1}] [{g + 1}, {w - 1}] seed at 0", {0: both + [(0, 0, 255)]}, {0: [(0, g - 1)]}))
        rows.append((f"runs [0, {g - 1}] [{g + 1}, {w - 1}] seed at {w - 1}", {0: both + [(w - 1, w - 1, 255)]}, {0: [(g + 1, w - 1)]}))
    for s, c in ((w - 1, 0), (0, w - 1)):
        rows.append((f"no wrap: strong at {s}, candidates at {c} in this row and the next", {0: [(c, c, 128), (s, s, 255)], 1: [(c, c, 128)]}, {0: [(s, s)]}))
    per_frame = len(range(1, ROW_FRAME_H - 1, 3))
    nframes = (len(rows) + per_frame - 1) // per_frame
    maps = np.zeros((nframes, ROW_FRAME_H, w), np.uint8)
    want = np.zeros_like(maps)
    cases = []
    for i, (kind, draw, promoted) in enumerate(rows):
        f, r = i // per_frame, 1 + 3 * (i % per_frame)
        for dy, spans in draw.items():
            for c0, c1, v in spans:
                maps[f, r + dy, c0:c1 + 1] = v
        for dy, spans in promoted.items():
            for c0, c1 in spans:
                want[f, r + dy, c0:c1 + 1] = 255
        cases.append((f, r, kind))
    return _frozen(maps), _frozen(want), tuple(cases)


def case_at(cases, frame, row):
    """The (frame, row, kind) of row_cases / seam_cases that owns map row `row` of `frame` (a failure message names it)."""
    best = None
    for c in cases:
        if c[0] == frame and abs(c[1] - row) <= 1 and (best is None or abs(c[1] - row) < abs(best[1] - row)):
            best = c
    return best


# ---- the seam between two column panels ----------------------------------------------------------------------------------------
def seam_cases(w, h, tile_rows, waves):
    """(maps, expected, cases) for the column halos of a frame wider than one panel (k_hyst's lmask / rmask): a strong pixel at
    (y, 2047) beside a lone candidate at (y + dy, 2048), and the mirror image with the strong pixel at (y, 2048) and the candidate
    at (y + dy, 2047) -- y at the first and last rows of a wave, a tile and the frame, dy in -1, 0, 1.  The candidate is promoted
    in every case.  cases: (frame, y, kind); cases of one frame keep two empty rows between them."""
    assert w > PANEL_COLS + 1
    tile = tile_rows * waves
    ys = sorted({y for y in (0, 1, tile_rows - 1, tile_rows, tile - 1, tile, tile + 1, h - 2, h - 1) if 0 <= y < h})
    frames, cases = [], []   # frames: the occupied rows of each
    for strong_col, cand_col in ((PANEL_COLS - 1, PANEL_COLS), (PANEL_COLS, PANEL_COLS - 1)):
        for dy in (-1, 0, 1):
            for y in ys:
                if not 0 <= y + dy < h:
                    continue
                lo, hi = min(y, y + dy), max(y, y + dy)
                for f, used in enumerate(frames):
                    if all(u < lo - 2 or u > hi + 2 for u in used):
                        break
                else:
                    f = len(frames)
                    frames.append(set())
                frames[f].update((lo, hi))
                cases.append((f, y, f"strong at ({y}, {strong_col}), candidate at ({y + dy}, {cand_col})", strong_col, cand_col, dy))
    maps = np.zeros((len(frames), h, w), np.uint8)
    for f, y, _, strong_col, cand_col, dy in cases:
        maps[f, y + dy, cand_col] = 128
        maps[f, y, strong_col] = 255
    want = np.where(maps != 0, 255, 0).astype(np.uint8)
    return _frozen(maps), _frozen(want), tuple(c[:3] for c in cases)
