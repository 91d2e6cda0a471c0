"""The maps of tests/test_gpu_hyst_dense_rows.py (tests/hyst_dense_maps.py) against the oracle, without a GPU: that they reach
both ways of k_hyst's write-back.  HYST_ROW_FULL is read from the source (canny_params.h), so a change of the constant that
leaves a map on one side of it only fails here.

Per map, from the oracle's planes before and after (changed 16-px groups per row and 2048-column panel):
- the maps that carry their promotion from one seed ("alternate", "dense", "threshold") promote every candidate, so the change
  passes through every row tile, whatever the tile height;
- widths that hold HYST_ROW_FULL groups: "alternate", "threshold" and "strong" have a row at or above the constant and a changed
  row below it; "dense" has every row of the first panel at or above it -- that is the variant (it cannot also have a row below);
  "threshold" has exactly HYST_ROW_FULL - 1, HYST_ROW_FULL and HYST_ROW_FULL + 1 changed groups in the rows 5, 6 and 7;
- width 33 (three groups a row) lies below the constant in every row: it is there for the ragged last group of the other way.
The iid-noise frames of the pipelined leg: at 1920 columns most rows are at or above the constant and some below; at 256
columns (16 groups) none can be."""
import functools

import numpy as np
import pytest

import hyst_dense_maps as D
from cudacam_amd import synth

FULL = D.row_full()
SMALL_W = 16 * (FULL + 8)   # "16 k for a small k": the smallest k that leaves room for FULL + 1 groups and a sparse row's tail
WIDTHS = [SMALL_W, 33, 1000, 1920, 1984, 2049]
HEIGHTS = [31, 64, 65, 70]


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import oracle as O
    O.build()
    return O


def test_the_constant_is_in_the_measured_range():
    assert 16 <= FULL <= 64


@pytest.mark.parametrize("h", HEIGHTS)
@pytest.mark.parametrize("w", WIDTHS)
def test_maps_reach_both_paths(w, h):
    maps, names = D.batch(w, h, FULL)
    assert np.isin(maps, (0, 128, 255)).all() and not maps.flags.writeable
    holds_full = min(w, D.PANEL_COLS) >= 16 * FULL
    assert holds_full == (w != 33)
    assert (("threshold", "top") in names) == holds_full
    for t, (variant, seed_at) in zip(maps, names):
        want = _oracle().hysteresis(t)
        g = D.changed_groups(t, want)
        what = f"{variant} seeded at the {seed_at}, {w} x {h}"
        if variant != "strong":
            assert np.array_equal(want, np.where(t != 0, 255, 0)), f"{what}: a candidate is not promoted"
            assert (g[:, 0] > 0).all(), f"{what}: a row does not change"
        changed = g[g > 0]
        if not holds_full:
            assert (changed < FULL).all(), what
            continue
        assert (g >= FULL).any(), f"{what}: no row at or above HYST_ROW_FULL = {FULL}"
        if variant == "dense":
            assert (g[:, 0] >= FULL).all(), what
        else:
            assert (changed < FULL).any(), f"{what}: no changed row below HYST_ROW_FULL = {FULL}"
        if variant == "threshold":
            assert list(g[5:8, 0]) == [FULL - 1, FULL, FULL + 1], f"{what}: rows 5 .. 7 change {list(g[5:8, 0])} groups"
            if h > 40:
                assert list(g[37:40, 0]) == [FULL - 1, FULL, FULL + 1], what
        if w > D.PANEL_COLS and variant != "strong":   # the second panel holds one column: one group, in the dense rows
            assert g[:, 1].max() == 1


@pytest.mark.parametrize("w", [256, 1920])
def test_noise_frames_of_the_pipelined_leg(w):
    h = 70
    for seed in (41, 42):
        st = _oracle().canny_r(synth.noise(w, h, seed), 10, 40, stages=True)
        g = D.changed_groups(np.where(st["thresh"] == 255, 255, 0).astype(np.uint8), st["edges"])
        if w == 256:
            assert g.max() < FULL and (g > 0).any()
        else:
            assert (g >= FULL).sum() > h // 2 and ((g > 0) & (g < FULL)).any(), f"noise {w} x {h} seed {seed}: rows at or above {FULL}: {(g >= FULL).sum()}, below: {((g > 0) & (g < FULL)).sum()}"
