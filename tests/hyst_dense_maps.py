"""Tri-state maps (0 / 128 / 255) whose rows change in MANY 16-px groups, for k_hyst's write-back (cudacam_amd/csrc/hyst.hip),
pure numpy.

When k_hyst patches a map that already shows the strong plane, a changed row goes one of two ways: fewer than HYST_ROW_FULL
(canny_params.h) changed 16-px groups are queued and expanded 64 at a time; at least that many and the row is written whole
(expand_rows).  A launch patches from launch 1 on (hc_hysteresis_device) or from launch 0 on (pipelined runs with a provisional
map), so the maps here carry their promotion from ONE strong pixel, in the first or the last row, through every row: the row
tile that holds the seed is written by launch 0, every other tile is patched by a later launch, with all the changed groups
of a row in one launch.

Row kinds:
- dense: candidate runs over the whole row but two 1-px gaps (whose columns move from row to row): every group changes;
- sparse: single candidates at column 1 and below the gaps of the row above -- each touches the runs above and below -- and a
  short run [w - 4, w - 2]: four groups change at most;
- exact(k): one run over exactly the first k groups.
Variants: "alternate" (sparse, dense, sparse, ...), "dense" (every row), "threshold" (alternate, with exact(FULL - 1), exact(FULL),
exact(FULL + 1) in the rows 5 .. 7 and, where the frame has them, 37 .. 39) and "strong" (alternate, but the single pixels of
the sparse rows are strong from the start: every run is touched by a strong pixel of the row above, nothing comes from afar).

Every generator returns read-only arrays."""
import os
import re

import numpy as np

PANEL_COLS = 2048
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def row_full():
    """HYST_ROW_FULL as committed (canny_params.h)"""
    src = open(os.path.join(_ROOT, "cudacam_amd", "csrc", "canny_params.h")).read()
    return int(re.search(r"#define HC_HYST_ROW_FULL (\d+)", src).group(1))


def _gaps(w, r):
    k = r % 5
    return 5 + 3 * k, w // 2 + 3 * k


def _dense_row(t, r):
    w = t.shape[1]
    t[r, :] = 128
    for g in _gaps(w, r):
        if 0 <= g < w:
            t[r, g] = 0


def _sparse_row(t, r, value):
    w = t.shape[1]
    for c in (1,) + _gaps(w, r - 1):
        if 0 <= c < w:
            t[r, c] = value
    t[r, max(w - 4, 0):max(w - 1, 1)] = 128


def dense_map(w, h, variant, seed_at, full):
    """One w x h map of `variant` ("alternate", "dense", "threshold", "strong") with its seed in the first row (seed_at "top")
    or the last ("bottom"); `full` = HYST_ROW_FULL (only "threshold" uses it; it needs w >= 16 * (full + 1))."""
    assert variant in ("alternate", "dense", "threshold", "strong") and seed_at in ("top", "bottom") and w >= 33
    t = np.zeros((h, w), np.uint8)
    for r in range(h):
        if variant == "dense" or r % 2 == 1:
            _dense_row(t, r)
        else:
            _sparse_row(t, r, 255 if variant == "strong" else 128)
    if variant == "threshold":
        assert w >= 16 * (full + 1) and h >= 9
        for r0 in (5, 37):
            if r0 + 3 < h:
                for i, k in enumerate((full - 1, full, full + 1)):
                    t[r0 + i, :] = 0
                    t[r0 + i, :16 * k] = 128
                for r in (r0 - 1, r0 + 3):   # the sparse rows around them: a candidate at column 1 joins them to the runs
                    t[r, :] = 0
                    _sparse_row(t, r, 128)
    t[0 if seed_at == "top" else h - 1, 1] = 255
    t.setflags(write=False)
    return t


def batch(w, h, full):
    """(maps, names): the frames of one call at w x h -- every variant the width can hold, seeded at the top and at the bottom"""
    names = [(v, s) for v in ("alternate", "dense", "threshold") for s in ("top", "bottom") if v != "threshold" or (w >= 16 * (full + 1) and h >= 9)]
    names.append(("strong", "top"))
    maps = np.stack([dense_map(w, h, v, s, full) for v, s in names])
    maps.setflags(write=False)
    return maps, tuple(names)


def changed_groups(t, want):
    """(h, panels) int: the 16-px groups of each row, per 2048-column panel, in which `want` (0 / 255) has a pixel that is not
    strong in the tri-state map t -- what a launch of k_hyst that changes the whole row at once counts for it"""
    h, w = t.shape
    ch = (want == 255) & (t != 255)
    wp = (w + PANEL_COLS - 1) // PANEL_COLS * PANEL_COLS
    g = np.zeros((h, wp), bool)
    g[:, :w] = ch
    return g.reshape(h, wp // PANEL_COLS, PANEL_COLS // 16, 16).any(axis=3).sum(axis=2)
