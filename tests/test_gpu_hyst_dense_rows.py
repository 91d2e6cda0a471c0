"""k_hyst's write-back (cudacam_amd/csrc/hyst.hip) on rows that change in many 16-px groups, bit for bit against the oracle.

A launch that patches a map writes a changed row whole when at least HYST_ROW_FULL of its groups changed (expand_rows, the
code that also writes every row of a launch on planes the map does not show yet) and group by group through the LDS queue
otherwise.  The maps (tests/hyst_dense_maps.py; tests/test_hyst_dense_maps_cpu.py shows on the CPU that they have rows on both
sides of the constant) carry their promotion from one seed through every row tile, so every tile but the seed's is patched.

Map leg (hc_hysteresis_device): every variant the width holds in one call, seeded at the top and at the bottom;
widths 16 k (k = HYST_ROW_FULL + 8), 33 and 1000 (a ragged last group), 1920, 1984 (the widest one-panel frame), 2049 (two
panels, the second one column wide); heights 31, 64, 65 and 70 (rows on both sides of a wave and of a tile boundary, a wave
with fewer than 32 rows, one with a single row); three output views, each with a workgroup shape of 32-row waves:
- tight, 32 rows x 2 waves (the shape beside the front kernel; one-panel frames: k_hyst_loop);
- a pitch that is a multiple of 4 but not of 16 (the dword stores), 32 rows x 1 wave (a tile boundary every 32 rows);
- an ROI at an odd byte offset of a larger buffer, 32 rows x 2 waves without the looping kernel.
Every output buffer is pre-filled with 0xA5 and every byte outside the view must still hold it.
Pipelined leg (hc_run_device, provisional map, launch 0 patches): iid-noise frames at 10 / 40, batch 2, three runs
rotating two output buffers, 256 x 70 (16 groups a row: the queue), 1000 x 70 and 1920 x 70 (whole rows; 1000: the ragged
group), at the default shape and at 32 x 2."""
import functools

import numpy as np
import pytest

import hyst_dense_maps as D
from cudacam_amd import api, synth

pytestmark = pytest.mark.gpu

FULL = D.row_full()
SMALL_W = 16 * (FULL + 8)
WIDTHS = [SMALL_W, 33, 1000, 1920, 1984, 2049]
HEIGHTS = [31, 64, 65, 70]
FILL = 0xA5
# view -> (HC_OPT_TEST_HYST_GEOM, HC_OPT_TEST_HYST_LOOP or None)
VIEWS = {"tight": (3202, None), "pitched": (3201, None), "roi": (3202, 0)}


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import oracle as O
    O.build()
    return O


@functools.lru_cache(maxsize=None)
def _batch(w, h):
    maps, names = D.batch(w, h, FULL)
    want = np.stack([_oracle().hysteresis(t) for t in maps])
    want.setflags(write=False)
    return maps, want, names


def _view(view, n, h, w):
    """(bytes of the buffer, offset of the view, pitch, frame stride)"""
    if view == "tight":
        return n * h * w, 0, w, w * h
    w4 = (w + 3) // 4 * 4
    if view == "pitched":
        pitch = w4 + 4 if (w4 + 4) % 16 else w4 + 8
        return n * h * pitch, 0, pitch, pitch * h
    pitch = w4 + 24
    return n * (h + 4) * pitch, 2 * pitch + 3, pitch, (h + 4) * pitch


def _check(buf, off, pitch, fs, want, what, names=None):
    n, h, w = want.shape
    idx = (off + np.arange(n)[:, None, None] * fs + np.arange(h)[None, :, None] * pitch + np.arange(w)[None, None, :]).reshape(-1)
    got = buf[idx].reshape(n, h, w)
    bad = np.argwhere(got != want)
    if bad.size:
        f, y, x = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} pixels differ, first at (row, col) ({y}, {x}) of frame {f} {names[f] if names else ''}: got {got[f, y, x]}, want {want[f, y, x]}")
    outside = np.ones(buf.shape, bool)
    outside[idx] = False
    assert (buf[outside] == FILL).all(), f"{what}: {int((buf[outside] != FILL).sum())} bytes outside the view were written"


@pytest.mark.parametrize("h", HEIGHTS)
@pytest.mark.parametrize("w", WIDTHS)
def test_maps(w, h):
    import torch
    maps, want, names = _batch(w, h)
    n = len(maps)
    ip = (w + 3) // 4 * 4
    host = np.zeros((n, h, ip), np.uint8)
    host[:, :, :w] = maps
    d_in = torch.from_numpy(host).cuda()
    for view, (code, loop) in VIEWS.items():
        size, off, pitch, fs = _view(view, n, h, w)
        d_out = torch.full((size,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with api.Context(w, h, 1, n) as ctx:
            ctx.set_option(api.OPT_TEST_HYST_GEOM, code)
            if loop is not None:
                ctx.set_option(api.OPT_TEST_HYST_LOOP, loop)
            ctx.hysteresis_device(d_in.data_ptr(), ip, ip * h, d_out.data_ptr() + off, pitch, fs, n)
            ctx.sync()
            s = ctx.hysteresis_schedule()
            assert (s["tile_rows"], s["waves"]) == (code // 100, code % 100), s
            if loop is not None:
                assert s["loop"] == loop, s
        _check(d_out.cpu().numpy(), off, pitch, fs, want, f"{w} x {h} {view} shape {code}", names)


@functools.lru_cache(maxsize=None)
def _noise(w, h):
    frames = np.stack([synth.noise(w, h, 41), synth.noise(w, h, 42)])
    want = _oracle().canny_r_batch(frames, 10, 40, threads=2)
    want.setflags(write=False)
    return frames, want


@pytest.mark.parametrize("code", [0, 3202])
@pytest.mark.parametrize("w", [256, 1000, 1920])
def test_noise_pipelined(w, code):
    import torch
    h = 70
    frames, want = _noise(w, h)
    d_fwd = torch.from_numpy(frames).cuda()
    d_rev = torch.from_numpy(frames[::-1].copy()).cuda()
    outs = [torch.full((2 * h * w,), FILL, dtype=torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    with api.Context(w, h, 1, 2) as ctx:
        if code:
            ctx.set_option(api.OPT_TEST_HYST_GEOM, code)
        ctx.set_option(api.OPT_PIPELINE, 1)
        for run, d_in in enumerate((d_rev, d_fwd, d_fwd)):   # outputs 0, 1, 0: the third run patches a map over other content
            ctx.run_device(d_in.data_ptr(), w, w * h, outs[run % 2].data_ptr(), w, w * h, 2)
            if run == 0:   # every map is checked: the first run's before the third overwrites it
                ctx.sync()
                _check(outs[0].cpu().numpy(), 0, w, w * h, want[::-1], f"noise {w} x {h} shape {code}, run 0")
        ctx.sync()
    for b in range(2):
        _check(outs[b].cpu().numpy(), 0, w, w * h, want, f"noise {w} x {h} shape {code}, output {b}")
