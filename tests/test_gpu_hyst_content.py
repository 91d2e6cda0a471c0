"""k_hyst (cudacam_amd/csrc/hyst.hip) on content aimed at how it propagates -- the maps of tests/hyst_maps.py, shown not to be
vacuous by tests/test_hyst_maps_cpu.py -- bit for bit against oracle.hysteresis, through hc_hysteresis_device as in
tests/test_gpu_hyst_shapes.py: the output pre-filled with 77, a fresh context per case, the pitch padded to a multiple of 4,
the schedule checked where a shape is forced.

- row_cases: row_fill's carry look-ahead (runs that start / end at bit 0 / 31 of a lane, runs of whole lanes, a single 0 at a
  lane boundary, the seed at either end or in the middle) and row_dilate's step across lanes and its ends (no wrap).
- seam_cases: the column halos of a two-panel frame at every row offset, at the first / last rows of wave, tile and frame.
- vertical serpentines: one wave boundary per column and direction, so one round of the tile loop each -- well within
  HYST_ROUND_CAP rounds, beyond it (a tile that runs out of rounds must leave itself work for another launch), across row
  tiles (launches), and with a slow tile beside a fast one in k_hyst_loop.
- spirals: propagation up, down, left and right through every neighbouring tile."""
import functools
import time

import numpy as np
import pytest

import hyst_maps as M
from cudacam_amd import api

pytestmark = pytest.mark.gpu

DEFAULT_SHAPE = (16, 8)   # what a single frame gets (hyst_tile_geometry); every case that relies on it checks the schedule


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import oracle as O
    O.build()
    return O


def _want(maps):
    """oracle.hysteresis of (n, h, w) maps, read-only"""
    out = np.stack([_oracle().hysteresis(m) for m in maps])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _serpentine(name):
    w, h, r0, r1, ncols, shape = M.SERPENTINES[name]
    t, path = M.vertical_serpentine(w, h, r0, r1, ncols)
    return t, _want(t[None])[0], path, shape


@functools.lru_cache(maxsize=None)
def _rows(w):
    maps, _, cases = M.row_cases(w)
    return maps, _want(maps), cases


@functools.lru_cache(maxsize=None)
def _seams(w, h, tr, waves):
    maps, _, cases = M.seam_cases(w, h, tr, waves)
    return maps, _want(maps), cases


@functools.lru_cache(maxsize=None)
def _spiral(w, h, seed_at):
    t, _ = M.spiral(w, h, 4, seed_at)
    return t, _want(t[None])[0]


def _hysteresis(ctx, maps):
    """(n, h, w) tri-state maps through hc_hysteresis_device: the edge maps, and the wall time of call + sync"""
    import torch
    n, h, w = maps.shape
    pitch = (w + 3) // 4 * 4
    host = np.zeros((n, h, pitch), np.uint8)
    host[:, :, :w] = maps
    d_in = torch.from_numpy(host).cuda()
    d_out = torch.full((n, h, pitch), 77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ctx.hysteresis_device(d_in.data_ptr(), pitch, pitch * h, d_out.data_ptr(), pitch, pitch * h, n)
    ctx.sync()
    ms = (time.perf_counter() - t0) * 1e3
    got = d_out.cpu().numpy()
    assert (got[:, :, w:] == 77).all(), "bytes between the rows were written"
    return got[:, :, :w], ms


def _check_shape(ctx, shape, w):
    s = ctx.hysteresis_schedule()
    assert (s["tile_rows"], s["waves"]) == tuple(shape), f"the run did not get the shape {shape}: {s}"
    assert s["panels"] == M.panels(w), s
    return s


def _diff(got, want, family, cases=None):
    bad = np.argwhere(got != want)
    if bad.size == 0:
        return
    f, y, x = (int(v) for v in bad[0])
    case = f"frame {f}" if cases is None else f"case {M.case_at(cases, f, y)}"
    raise AssertionError(f"{family}: {len(bad)} pixels differ, first at (row, col) ({y}, {x}) of {case}: got {got[f, y, x]}, want {want[f, y, x]}")


def _report(ctx, what, ms):
    print(f"{what}: {ms:.2f} ms, schedule {ctx.hysteresis_schedule()} info {ctx.hysteresis_info()} totals {ctx.hysteresis_totals()}")


@pytest.mark.parametrize("variant", ["defaults", "one_launch"])
@pytest.mark.parametrize("w", [2048, 1984, 300, 2112, 2049])
def test_row_cases(w, variant):
    maps, want, cases = _rows(w)
    n, h = maps.shape[:2]
    with api.Context(w, h, 1, n) as ctx:
        if variant == "one_launch":   # a single queued launch: whatever crosses the panel seam is finished by the host continuation
            ctx.set_tuning(0, 1)
        got, ms = _hysteresis(ctx, maps)
        s = _check_shape(ctx, DEFAULT_SHAPE, w)
        _report(ctx, f"row_cases {w} x {h} x {n} {variant}", ms)
        if variant == "one_launch":
            assert s["launches"] == 1, s
            if w > M.PANEL_COLS:   # (the runs over column 2048)
                assert ctx.hysteresis_info()[1] == 1, "the host continuation did not run"
    _diff(got, want, f"row_cases width {w} {variant}", cases)


@pytest.mark.parametrize("variant", ["defaults", "lists_grid1", "per_tile"])
@pytest.mark.parametrize("code", [3208, 1608, 3202])
def test_seam_cases(code, variant):
    tr, waves = code // 100, code % 100
    w, h = 2112, 2 * tr * waves + 9
    maps, want, cases = _seams(w, h, tr, waves)
    with api.Context(w, h, 1, len(maps)) as ctx:
        ctx.set_option(api.OPT_TEST_HYST_GEOM, code)
        if variant == "lists_grid1":
            ctx.set_option(api.OPT_TEST_HYST_LATE_GRID, 1)
        elif variant == "per_tile":
            ctx.set_option(api.OPT_TEST_HYST_LATE_GRID, -1)
        got, ms = _hysteresis(ctx, maps)
        s = _check_shape(ctx, (tr, waves), w)
        _report(ctx, f"seam_cases {code} {w} x {h} x {len(maps)} {variant}", ms)
        assert s["lists"] == (0 if variant == "per_tile" else 1), s
    _diff(got, want, f"seam_cases {code} {variant}", cases)


@pytest.mark.parametrize("name", ["short", "short_1984", "short_seam"])
def test_vertical_serpentine_within_the_cap(name):
    """Passes with a tile loop that gives up silently at the cap as well: these paths need fewer than half its rounds."""
    t, want, path, _ = _serpentine(name)
    h, w = t.shape
    with api.Context(w, h, 1, 1) as ctx:
        got, ms = _hysteresis(ctx, t[None])
        _check_shape(ctx, DEFAULT_SHAPE, w)
        print(f"{name}: {M.wave_crossings(path, *DEFAULT_SHAPE)} wave crossings")
        _report(ctx, f"vertical serpentine {name} {w} x {h}", ms)
    _diff(got, want[None], f"vertical serpentine {name}")


@pytest.mark.parametrize("name,loop", [("long", 1), ("long", 0), ("long_1984", 1), ("long_1984", 0), ("long_3216", 0), ("long_3216_1984", 0)])
def test_vertical_serpentine_beyond_the_cap(name, loop):
    """One tile whose path needs more sequential rounds of the tile loop than the HYST_ROUND_CAP = 4096 a launch has: at the
    default shape 7 wave boundaries x 1023 columns = 7161 (2048 wide: two panels, the kernels with the panel code) and x 992
    columns = 6944 (1984 wide: one panel, k_hyst_loop unless `loop` is 0), at 32 rows x 16 waves 15 x 1023 = 15345 and 15 x 992
    = 14880 (that shape has no looping kernel).  The tile's first and last rows and columns are empty, so no boundary ever
    changes: a tile that leaves the loop at the cap has to say itself that it is not done -- the launch's flag, and a reason
    word (in the list modes also a list entry) that reopens its rows in the next launch.

    Before the tile did that, the loop left at the cap without a word and the run ended as converged with the rest of the path
    unpromoted: measured once on the MI355X with the kernel as it was, all six cases failed, with 55 610 (long, either way),
    51 673 (long_1984, either way), 383 218 (long_3216) and 367 377 (long_3216_1984) pixels 0 instead of 255.  Now the cases take
    2, 2 and 4 launches with work (46 to 55 ms, and 181 to 216 ms at 16 waves: ~15 000 rounds of one workgroup).  DESIGN.md 3.3,
    "What costs rounds, what costs launches"."""
    t, want, path, shape = _serpentine(name)
    h, w = t.shape
    with api.Context(w, h, 1, 1) as ctx:
        if shape:
            ctx.set_option(api.OPT_TEST_HYST_GEOM, shape[0] * 100 + shape[1])
        if not loop:
            ctx.set_option(api.OPT_TEST_HYST_LOOP, 0)
        got, ms = _hysteresis(ctx, t[None])
        s = _check_shape(ctx, shape or DEFAULT_SHAPE, w)
        print(f"{name}: {M.wave_crossings(path, *(shape or DEFAULT_SHAPE))} wave crossings")
        _report(ctx, f"vertical serpentine {name} {w} x {h} loop {loop}", ms)
        assert s["loop"] == (loop if M.panels(w) == 1 and not shape else 0), s
    _diff(got, want[None], f"vertical serpentine {name} loop {loop}")


def test_vertical_serpentine_across_row_tiles():
    """31 columns over the full height of three row tiles and a partial fourth: every column crosses every tile boundary, 93
    crossings, one launch each -- far more than a run queues, so the host continuation finishes it."""
    tr, waves = DEFAULT_SHAPE
    w, h = 64, 3 * tr * waves + 9
    t, path = M.vertical_serpentine(w, h, 0, h, 31)
    want = _want(t[None])
    with api.Context(w, h, 1, 1) as ctx:
        got, ms = _hysteresis(ctx, t[None])
        s = _check_shape(ctx, DEFAULT_SHAPE, w)
        print(f"{M.tile_crossings(path, tr, waves)} tile crossings, {s['launches']} launches queued")
        _report(ctx, f"vertical serpentine across row tiles {w} x {h}", ms)
        assert M.tile_crossings(path, tr, waves) > 2 * s["launches"]
        assert ctx.hysteresis_info()[1] >= 1, "the host continuation did not run"
    _diff(got, want, "vertical serpentine across row tiles")


def test_slow_tile_beside_a_fast_one():
    """Two tiles in k_hyst_loop: the long serpentine keeps the top one in its tile loop for thousands of rounds while the bottom
    one -- a seed with a three-pixel stub -- is done at once and waits at the device-wide barrier.  Whether the barrier's
    bounded wait runs out (the run is then handed to the host) depends on the clocks, so only the map is asserted: it must be
    exact either way.  Observed on the MI355X (the schedule / info / totals this prints): the wait did run out, the host
    continuation ran (hysteresis_info() = (3, 1)), 46 ms in all.  1984 columns, not 2048: see hyst_maps.SERPENTINES."""
    w, h, r0, r1, ncols, _ = M.SERPENTINES["long_1984"]   # (one panel: 2048 columns would be two, without k_hyst_loop)
    t, _ = M.vertical_serpentine(w, 2 * h, r0, r1, ncols)
    t = t.copy()
    t[200, 100] = 255
    t[201:204, 100] = 128
    want = _want(t[None])
    assert (want[0, 200:204, 100] == 255).all()
    with api.Context(w, 2 * h, 1, 1) as ctx:
        got, ms = _hysteresis(ctx, t[None])
        s = _check_shape(ctx, DEFAULT_SHAPE, w)
        _report(ctx, f"slow tile beside a fast one {w} x {2 * h}", ms)
        assert s["loop"] == 1 and s["tiles"] == 2, s
    _diff(got, want, "slow tile beside a fast one")


@pytest.mark.parametrize("variant", ["defaults", "one_launch"])
@pytest.mark.parametrize("seed_at", ["outer", "centre"])
@pytest.mark.parametrize("w,h,code", [(300, 153, 0), (2112, 2 * 64 + 9, 3202)])
def test_spirals(w, h, code, seed_at, variant):
    t, want = _spiral(w, h, seed_at)
    with api.Context(w, h, 1, 1) as ctx:
        if code:
            ctx.set_option(api.OPT_TEST_HYST_GEOM, code)
        if variant == "one_launch":
            ctx.set_tuning(0, 1)
        got, ms = _hysteresis(ctx, t[None])
        s = _check_shape(ctx, (code // 100, code % 100) if code else DEFAULT_SHAPE, w)
        _report(ctx, f"spiral {w} x {h} seed {seed_at} {variant}", ms)
        if variant == "one_launch":
            assert s["launches"] == 1 and ctx.hysteresis_info()[1] == 1, s
    _diff(got, want[None], f"spiral {w} x {h} seed {seed_at} {variant}")
