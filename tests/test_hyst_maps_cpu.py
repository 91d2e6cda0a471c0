"""The maps of tests/test_gpu_hyst_content.py (tests/hyst_maps.py) against the oracle, without a GPU: every map is tri-state,
oracle.hysteresis promotes exactly what the case states (so no map is vacuous), the transposed map gives the transposed
result (the fixpoint is symmetric; this guards the generators, not the oracle), and the serpentines stand where the GPU test
needs them relative to k_hyst's round cap -- read from the source, so a change of the cap or of the default shape that moves
a case to the other side of it fails here."""
import functools
import os
import re

import numpy as np
import pytest

import hyst_maps as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEAM_SHAPES = [(32, 8), (16, 8), (32, 2)]   # test_seam_cases' shapes (3208, 1608, 3202)


@functools.lru_cache(maxsize=None)
def _params():
    return open(os.path.join(ROOT, "cudacam_amd", "csrc", "canny_params.h")).read()


def _round_cap():
    return int(re.search(r"constexpr int HYST_ROUND_CAP = (\d+);", _params()).group(1))


def _default_shape():
    """(tile_rows, waves) of a run of a few frames (hyst_tile_geometry)"""
    m = re.search(r"if \(frames_x_rows < 128 \* 1024\) \{ \*tile_rows = (\d+); \*waves = (\d+); \}", _params())
    return int(m.group(1)), int(m.group(2))


def _tri_state(t):
    assert t.dtype == np.uint8 and not t.flags.writeable
    assert np.isin(t, (0, 128, 255)).all()


def _transposes(O, t, want):
    assert np.array_equal(O.hysteresis(np.ascontiguousarray(t.T)).T, want)


def _all_strong(t):
    return np.where(t != 0, 255, 0).astype(np.uint8)


def _is_path(path):
    p = np.asarray(path)
    assert len(set(path)) == len(path), "the path visits a pixel twice"
    assert (np.abs(np.diff(p, axis=0)).max(axis=1) == 1).all(), "consecutive pixels of the path are not 8-neighbours"


def test_the_kernel_loop_uses_the_named_cap():
    src = open(os.path.join(ROOT, "cudacam_amd", "csrc", "hyst.hip")).read()
    assert _round_cap() > 0
    assert len(re.findall(r"for \(round = 0; round < HYST_ROUND_CAP; \+\+round\)", src)) == 1


@pytest.mark.parametrize("name", sorted(M.SERPENTINES))
def test_vertical_serpentines(oracle, name):
    w, h, r0, r1, ncols, shape = M.SERPENTINES[name]
    t, path = M.vertical_serpentine(w, h, r0, r1, ncols)
    _tri_state(t)
    _is_path(path)
    assert path[0] == (r0, 1) and t[r0, 1] == 255 and np.count_nonzero(t == 255) == 1
    assert np.count_nonzero(t) == len(path) == ncols * (r1 - r0) + ncols - 1
    rows, cols = np.asarray(path).T
    assert rows.min() == r0 and rows.max() == r1 - 1 and cols.max() == 2 * ncols - 1
    want = oracle.hysteresis(t)
    assert np.array_equal(want, _all_strong(t)), "the oracle does not promote the whole path"
    weak = t.copy()
    weak[r0, 1] = 128
    assert not oracle.hysteresis(weak).any(), "something but the seed promotes the path"
    _transposes(oracle, t, want)
    # where the case stands relative to the cap, at the shape it runs with: conditions on the input, not measurements
    tr, waves = shape or _default_shape()
    assert h <= tr * waves and M.tile_crossings(path, tr, waves) == 0, "the path is meant to stay inside one row tile"
    need, cap = M.wave_crossings(path, tr, waves), _round_cap()
    per_column = (r1 - 1) // tr - r0 // tr
    assert need == per_column * ncols
    if name.startswith("short"):
        assert 0 < need < cap / 2, f"{name}: {need} rounds, cap {cap}: no longer well within the cap"
    else:
        assert need > 1.5 * cap, f"{name}: {need} rounds, cap {cap}: no longer reaches the cap"
    if w > M.PANEL_COLS:
        assert cols.max() > M.PANEL_COLS + 32, "the path does not cross the panel seam"


def test_panels():
    assert [M.panels(w) for w in (300, 1984, 1985, 2048, 2049, 2112, 3968, 3969)] == [1, 1, 2, 2, 2, 2, 2, 4]
    assert M.panels(M.ONE_PANEL_MAX_W) == 1 and M.panels(M.ONE_PANEL_MAX_W + 1) == 2
    src = open(os.path.join(ROOT, "cudacam_amd", "csrc", "host_plan.h")).read()   # the rule this restates
    assert "std::max<size_t>((size_t)(W + 31) / 32, ((size_t)((W + STRIP_W - 1) / STRIP_W) * 31 + 3) / 4)" in src
    assert "need <= 64 ? 64 : need <= 128 ? 128 : 256" in src and re.search(r"constexpr int STRIP_W = \(LANES - 2\) \* PX_PER_LANE;  // 248", _params())


def test_crossings_count_waves_and_tiles():
    path = tuple((y, 1) for y in range(0, 40)) + ((39, 2),) + tuple((y, 3) for y in range(39, 29, -1))
    # rows 0..39 down, 39..30 up; waves of 8 rows, tiles of 2 waves: boundaries at 8 (wave), 16 (tile), 24 (wave), 32 (tile)
    assert M.wave_crossings(path, 8, 2) == 2 and M.tile_crossings(path, 8, 2) == 2 + 1
    assert M.wave_crossings(path, 16, 8) == 2 + 1 and M.tile_crossings(path, 16, 8) == 0


def test_across_row_tiles_serpentine(oracle):
    tr, waves = _default_shape()
    w, h = 64, 3 * tr * waves + 9
    t, path = M.vertical_serpentine(w, h, 0, h, 31)
    _tri_state(t)
    _is_path(path)
    want = oracle.hysteresis(t)
    assert np.array_equal(want, _all_strong(t))
    _transposes(oracle, t, want)
    assert M.tile_crossings(path, tr, waves) == 3 * 31   # far more than the launches a run queues (test_gpu_hyst_content)


@pytest.mark.parametrize("seed_at", ["outer", "centre"])
@pytest.mark.parametrize("w,h", [(300, 153), (2112, 2 * 64 + 9)])
def test_spirals(oracle, w, h, seed_at):
    t, path = M.spiral(w, h, 4, seed_at)
    _tri_state(t)
    _is_path(path)
    assert t[path[0]] == 255 and np.count_nonzero(t == 255) == 1 and np.count_nonzero(t) == len(path)
    # 1 px wide, arms apart: a pixel of the path touches its two neighbours on the path, and next to a corner a third
    c = np.pad((t != 0).astype(np.int32), 1)
    nbrs = sum(c[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))
    assert nbrs[t != 0].max() <= 3 and nbrs[t != 0].min() >= 1
    rows, cols = np.asarray(path).T
    assert rows.min() == 0 and rows.max() == h - 1 and cols.min() == 0 and cols.max() == w - 1
    inner = path[-1] if seed_at == "outer" else path[0]
    assert abs(inner[0] - h / 2) <= 8 and len(path) > w * h // 5, "the spiral does not reach the centre"
    # ... so it runs all four ways through every tile it passes: each direction has arms on both sides of the centre
    d = np.diff(np.asarray(path), axis=0)
    for step in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        assert np.count_nonzero((d == step).all(axis=1)) > h
    want = oracle.hysteresis(t)
    assert np.array_equal(want, _all_strong(t)), "the oracle does not promote the whole spiral"
    weak = t.copy()
    weak[path[0]] = 128
    assert not oracle.hysteresis(weak).any()
    _transposes(oracle, t, want)


@pytest.mark.parametrize("w", [2048, 1984, 300, 2112, 2049])
def test_row_cases(oracle, w):
    maps, want, cases = M.row_cases(w)
    _tri_state(maps)
    assert maps.shape == want.shape and maps.shape[1:] == (M.ROW_FRAME_H, w)
    assert len({(f, r) for f, r, _ in cases}) == len(cases) and all(r % 3 == 1 and 1 <= r < M.ROW_FRAME_H - 1 for _, r, _ in cases)
    kinds = [k for _, _, k in cases]
    ends = [e for e in (0, 1, 30, 31, 32, 33, 63, 64, 65, 1023, 1024, 2015, 2016, 2046, 2047, 2048, 2049, w - 2, w - 1) if e < w and (e < 2048 or w > 2048)]
    ends = sorted(set(ends))
    for a in ends:
        for b in ends:
            if a <= b:
                for s in (f"start {a}", f"end {b}", f"middle {(a + b) // 2}"):
                    assert f"run [{a}, {b}] seed at its {s}" in kinds
                assert (f"run [{a}, {b}] below a strong pixel at start - 1 {a - 1}" in kinds) == (a > 0)
                assert (f"run [{a}, {b}] below a strong pixel at end + 1 {b + 1}" in kinds) == (b < w - 1)
    for g in (31, 32, 63, 64, 1023, 1024, 2047, 2048):
        assert (f"runs [0, {g - 1}] [{g + 1}, {w - 1}] seed at 0" in kinds) == (g + 1 <= w - 1 and (g < 2047 or w > 2048))
    assert sum(k.startswith("no wrap") for k in kinds) == 2
    # cases cannot interact: between the rows two cases draw on lies an empty row
    used = maps.any(axis=2)
    owner = np.full(used.shape, -1)
    for i, (f, r, kind) in enumerate(cases):
        assert used[f, r], kind
        owner[f, r - 1:r + 2] = i
    assert (owner[used] >= 0).all()
    touching = used[:, 1:] & used[:, :-1]
    assert (owner[:, 1:][touching] == owner[:, :-1][touching]).all(), "two cases draw on neighbouring rows"
    # the oracle promotes what the case says: the seeded run and only it; nothing in the no-wrap rows
    for f in range(len(maps)):
        got = oracle.hysteresis(maps[f])
        bad = np.argwhere(got != want[f])
        assert bad.size == 0, f"width {w}: the oracle differs from what the case states at {tuple(bad[0])}: {M.case_at(cases, f, int(bad[0][0]))}"
        _transposes(oracle, maps[f], got)
    for f, r, kind in cases:
        promoted = (maps[f, r - 1:r + 2] == 128) & (want[f, r - 1:r + 2] == 255)
        left = (maps[f, r - 1:r + 2] == 128) & (want[f, r - 1:r + 2] == 0)
        if kind.startswith("no wrap"):
            assert not promoted.any() and np.count_nonzero(left) == 2
        elif kind.startswith("runs"):
            assert left.any() and (want[f, r] == 255).any(), kind   # one run filled, the other left
        else:
            assert not left.any(), kind
            assert promoted.any() or "seed at its" in kind, kind   # (a one-pixel run that is its own seed has no candidate left)


@pytest.mark.parametrize("tile_rows,waves", SEAM_SHAPES)
def test_seam_cases(oracle, tile_rows, waves):
    tile = tile_rows * waves
    w, h = 2112, 2 * tile + 9
    maps, want, cases = M.seam_cases(w, h, tile_rows, waves)
    _tri_state(maps)
    ys = sorted({0, 1, tile_rows - 1, tile_rows, tile - 1, tile, tile + 1, h - 2, h - 1})
    for strong_col, cand_col in ((2047, 2048), (2048, 2047)):
        for y in ys:
            for dy in (-1, 0, 1):
                kind = f"strong at ({y}, {strong_col}), candidate at ({y + dy}, {cand_col})"
                hits = [c for c in cases if c[2] == kind]
                assert len(hits) == (1 if 0 <= y + dy < h else 0), kind
                for f, cy, _ in hits:
                    assert cy == y and maps[f, y, strong_col] == 255 and maps[f, y + dy, cand_col] == 128
    assert np.count_nonzero(maps == 255) == np.count_nonzero(maps == 128) == len(cases)
    assert not maps[:, :, :2047].any() and not maps[:, :, 2049:].any()
    used = maps.any(axis=2)
    for f in range(len(maps)):   # cases of a frame cannot touch: runs of used rows are at most two rows long, two empty rows apart
        rows = np.flatnonzero(used[f])
        gaps = np.diff(rows)
        assert ((gaps == 1) | (gaps >= 3)).all() and not ((gaps[1:] == 1) & (gaps[:-1] == 1)).any()
        got = oracle.hysteresis(maps[f])
        assert np.array_equal(got, want[f]) and np.array_equal(got, _all_strong(maps[f])), "the oracle does not promote the lone candidates"
        _transposes(oracle, maps[f], got)
