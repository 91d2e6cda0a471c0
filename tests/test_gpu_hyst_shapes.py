"""Every workgroup shape k_hyst is compiled for (HYST_SHAPES, cudacam_amd/csrc/canny_params.h), run once in each of its
tile modes and in both panel forms, against the oracle.

The planner picks three of the eight shapes by its own rules; the others are reached through HC_OPT_TEST_HYST_GEOM (rows per
wave x 100 + waves per workgroup).  Geometry per shape: widths 300 (one panel, RD 64) and 2100 (two panels, RD 128, the seam
at column 2048), height 2 * tile_rows * waves + 9 -- three row tiles, the last one partial and shorter than one wave's rows
(waves with fewer than tile_rows rows, waves with none).  A fresh context per case, so no tile-level history applies.

Plain leg (hc_hysteresis_device, bit for bit against oracle.hysteresis, on a serpentine path from one seed and on candidate
clutter with sparse seeds): the defaults (a workgroup per tile, HYST_PER_TILE; width 2100: the lists); HC_OPT_TEST_HYST_LATE_GRID
1 (lists with one-workgroup grids: HYST_LIST_FIRST / HYST_LIST_LATE and the hand-on of entries beyond the grid) and -1 (a
workgroup per tile whatever the width); one queued launch (the host continuation); and, for the two shapes that have the
looping kernel, k_hyst_loop against the same run with HC_OPT_TEST_HYST_LOOP 0.
Pipelined leg (width 300, hc_run_device on two natural frames, against oracle.canny_r_batch): the mixed schedule, whose third
launch is HYST_PER_TILE_TO_LIST.

Both maps were checked on the CPU to make every row tile of every shape promote a candidate, at width 2100 on both sides of
column 2048 (`_maps` asserts it again): a kernel that ignored a neighbouring tile would fail.  The generators' parameters
are the ones named below; no other choice was needed at these sizes."""
import functools

import numpy as np
import pytest

from cudacam_amd import api, synth

pytestmark = pytest.mark.gpu

CODES = [3208, 3204, 3202, 3201, 3216, 1608, 1604, 1602]
WIDTHS = [300, 2100]
LOOPING = (1608, 3202)   # the shapes that also have k_hyst_loop
PANEL_COLS = 2048


def _shape(code):
    return code // 100, code % 100


def _height(code):
    tr, waves = _shape(code)
    return 2 * tr * waves + 9


@functools.lru_cache(maxsize=None)
def _maps(w, h, tile):
    """((name, tri-state map, expected edge map), ...) for a w x h frame whose row tiles are `tile` rows high"""
    from oracle import oracle as O
    O.build()
    out = []
    for name, thr in (("serpentine", synth.thresh_map_serpentine(w, h)), ("random", synth.thresh_map_random(w, h, 1000 + w + h, 0.45, 0.002))):
        want = O.hysteresis(thr)
        promoted = (thr == 128) & (want == 255)
        sides = [slice(0, PANEL_COLS), slice(PANEL_COLS, w)] if w > PANEL_COLS else [slice(0, w)]
        for r0 in range(0, h, tile):
            for cols in sides:
                assert promoted[r0:r0 + tile, cols].any(), f"{name} {w}x{h}: no candidate promoted in rows {r0}.. columns {cols}"
        thr.setflags(write=False)
        want.setflags(write=False)
        out.append((name, thr, want))
    return tuple(out)


def _hysteresis(ctx, thr):
    import torch
    h, w = thr.shape
    d_in = torch.from_numpy(thr.copy()).cuda()   # (the shared maps are read-only)
    d_out = torch.full((h, w), 77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.hysteresis_device(d_in.data_ptr(), w, w * h, d_out.data_ptr(), w, w * h, 1)
    ctx.sync()
    return d_out.cpu().numpy()


def _check_schedule(ctx, code, w):
    s = ctx.hysteresis_schedule()
    assert (s["tile_rows"], s["waves"]) == _shape(code), f"HC_OPT_TEST_HYST_GEOM {code} did not take effect: {s}"
    assert s["panels"] == (2 if w > PANEL_COLS else 1), s
    return s


def _diff(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} pixels differ, first at (row, col) {tuple(bad[0])}"


VARIANTS = ["defaults", "lists_grid1", "per_tile", "one_launch"]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("code", CODES)
def test_plain(oracle, code, w, variant):
    tr, waves = _shape(code)
    h = _height(code)
    for name, thr, want in _maps(w, h, tr * waves):
        with api.Context(w, h, 1, 1) as ctx:
            ctx.set_option(api.OPT_TEST_HYST_GEOM, code)
            if variant == "lists_grid1":
                ctx.set_option(api.OPT_TEST_HYST_LATE_GRID, 1)
            elif variant == "per_tile":
                ctx.set_option(api.OPT_TEST_HYST_LATE_GRID, -1)
            elif variant == "one_launch":
                ctx.set_tuning(0, 1)
            got = _hysteresis(ctx, thr)
            s = _check_schedule(ctx, code, w)
            print(f"{code} {w}x{h} {variant} {name}: {s} totals {ctx.hysteresis_totals()}")
            _diff(got, want, f"{code} {w}x{h} {variant} {name}")
            if variant == "defaults":
                assert s["loop"] == int(w == 300 and code in LOOPING), s
            if variant == "lists_grid1":
                assert s["lists"] == 1, s
            if variant == "per_tile":
                assert s["lists"] == 0, s
            if variant == "one_launch":
                assert s["launches"] == 1, s
                if name == "serpentine":   # the path crosses every row tile: one launch cannot finish it
                    assert ctx.hysteresis_totals()[1] == 1, "the host continuation did not run"


@pytest.mark.parametrize("code", LOOPING)
def test_looping_kernel_against_launches(oracle, code):
    """Width 300: the default takes k_hyst_loop, HC_OPT_TEST_HYST_LOOP 0 the same rounds as launches."""
    tr, waves = _shape(code)
    w, h = 300, _height(code)
    for name, thr, want in _maps(w, h, tr * waves):
        for loop in (1, 0):
            with api.Context(w, h, 1, 1) as ctx:
                ctx.set_option(api.OPT_TEST_HYST_GEOM, code)
                if not loop:
                    ctx.set_option(api.OPT_TEST_HYST_LOOP, 0)
                got = _hysteresis(ctx, thr)
                s = _check_schedule(ctx, code, w)
                assert s["loop"] == loop, s
                _diff(got, want, f"{code} {w}x{h} loop {loop} {name}")


@pytest.mark.parametrize("code", CODES)
def test_pipelined(oracle, code):
    import torch
    w, h = 300, _height(code)
    frames = np.stack([synth.natural(w, h, 500 + code), synth.natural(w, h, 501 + code)])
    want = oracle.canny_r_batch(frames, 10, 40, threads=2)
    d_fwd = torch.from_numpy(frames).cuda()
    d_rev = torch.from_numpy(frames[::-1].copy()).cuda()
    outs = [torch.full((2, h, w), 77, dtype=torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    with api.Context(w, h, 1, 2) as ctx:
        ctx.set_option(api.OPT_TEST_HYST_GEOM, code)
        ctx.set_option(api.OPT_PIPELINE, 1)
        for run, d_in in enumerate((d_rev, d_fwd, d_fwd)):   # outputs 0, 1, 0: the third run overwrites other content
            ctx.run_device(d_in.data_ptr(), w, w * h, outs[run % 2].data_ptr(), w, w * h, 2)
        ctx.sync()
        s = _check_schedule(ctx, code, w)
        print(f"{code} {w}x{h} pipelined: {s} totals {ctx.hysteresis_totals()}")
        assert s["lists"] == 2, s
    for b in range(2):
        for f in range(2):
            _diff(outs[b][f].cpu().numpy(), want[f], f"{code} {w}x{h} pipelined, output {b} frame {f}")
