"""hc_derivatives_device (k_deriv16) on the MI355X: the Sobel 3 / 5 / 7 and Scharr derivatives cv::Canny computes before its
NMS, bit for bit against tests/deriv_ref.py (anchored by tests/test_deriv_ref_cpu.py); caller views with guard bytes on the
input and on both outputs; the chain derivatives -> hc_run_gradients_device against HC_OPT_APERTURE 3 / 5 (no CPU reference
involved) and against the numpy restatement for 7 and Scharr."""
import os
import re

import numpy as np
import pytest

from cudacam_amd import api, synth
import canny_o_ext_ref as X
import deriv_ref as D
import view_arena as VA

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _param(name):
    src = open(os.path.join(ROOT, "cudacam_amd", "csrc", "canny_params.h")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


STRIP_W = _param("DERIV_STRIP_W")
CHUNK_ROWS = _param("DERIV_CHUNK_ROWS")
KSIZES = D.KSIZES


def _contents(w, h, ch, seed):
    """Five frames: uniform random, all 0, all 255, a checkerboard of 0 / 255 (extremes), a smoothed image (many ties)."""
    rng = np.random.default_rng(seed)
    shape = (h, w) if ch == 1 else (h, w, ch)
    rnd = rng.integers(0, 256, shape, dtype=np.uint8)
    cb = ((np.add.outer(np.arange(h), np.arange(w)) & 1) * 255).astype(np.uint8)
    sm = rng.integers(0, 256, shape).astype(np.int64)
    for ax in (0, 1):   # 5-tap box blur with replicated borders
        n = sm.shape[ax]
        sm = sum(np.take(sm, np.clip(np.arange(n) + k, 0, n - 1), axis=ax) for k in range(-2, 3))
    sm = (sm // 25).astype(np.uint8)
    if ch == 3:
        cb = np.stack([cb, 255 - cb, cb], -1)
    return np.stack([rnd, np.zeros(shape, np.uint8), np.full(shape, 255, np.uint8), cb, sm])


def _diff(got, want, what):
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    first = [(tuple(int(v) for v in p), int(got[tuple(p)]), int(want[tuple(p)])) for p in bad[:8]]
    raise AssertionError(f"{what}: {len(bad)} of {got.size} differ; first (pos, hip, ref): {first}")


SHAPES = sorted(set(
    [(1, 1), (2, 3), (5, 2), (7, 7), (64, 32), (700, 300)]
    + [(3, 5), (4, 5), (5, 5), (8, 3), (9, 4)]                                            # one lane group +- 1, two
    + [(STRIP_W - 1, 6), (STRIP_W, 6), (STRIP_W + 1, 6), (2 * STRIP_W + 1, 9)]            # strip boundaries
    + [(11, h) for h in range(1, 9)]                                                      # heights 1 .. ksize + 1
    + [(13, CHUNK_ROWS - 1), (13, CHUNK_ROWS), (13, CHUNK_ROWS + 1), (251, 2 * CHUNK_ROWS + 1)]))   # row chunks


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_shapes(w, h, ch):
    frames = _contents(w, h, ch, 1000 * w + h)
    with api.Context(w, h, ch, len(frames), api.MODE_O) as ctx:
        for ks in KSIZES:
            dx, dy = ctx.derivatives(frames, ks)
            assert dx.dtype == np.int16 and dx.shape == frames.shape
            wx, wy = D.sobel16_frames(frames, ks)
            _diff(dx, wx, f"dx ksize {ks} {w}x{h}x{ch}")
            _diff(dy, wy, f"dy ksize {ks} {w}x{h}x{ch}")


def _lead(pitch):
    return VA.round_up(pitch + 64, 16)   # the view's alignment is that of its base offset


def _run_view(ctx, frames, ks, in_pitch, in_fs, in_off, pitch, fs, out_off, fill="random", seed=0, want=None):
    """One call on guarded arenas: the views must hold the reference, every other byte of the three arenas must be unchanged."""
    import torch
    n, h, w = frames.shape[:3]
    ch = 1 if frames.ndim == 3 else 3
    a_in, off_in = VA.make_input(frames, in_pitch, in_fs, in_off, fill, lead=_lead(in_pitch), seed=seed)
    bx, gx = VA.make_output(n, h, 2 * ch * w, pitch, fs, out_off, lead=_lead(pitch), seed=seed + 1)
    by, gy = VA.make_output(n, h, 2 * ch * w, pitch, fs, out_off, lead=_lead(pitch), seed=seed + 2)
    d_in, d_x, d_y = (torch.from_numpy(v).cuda() for v in (a_in, bx, by))
    torch.cuda.synchronize()
    ctx.derivatives_device(d_in.data_ptr() + off_in, in_pitch, in_fs if in_fs else in_pitch * h, d_x.data_ptr() + gx.offset,
                           d_y.data_ptr() + gy.offset, pitch, fs if fs else pitch * h, n, ks)
    ctx.sync()
    wx, wy = want if want is not None else D.sobel16_frames(frames, ks)
    what = f"ksize {ks} {w}x{h}x{ch} in(pitch {in_pitch}, off {in_off}) out(pitch {pitch}, off {out_off})"
    VA.check_output(d_x.cpu().numpy(), bx, gx, wx, "dx " + what)
    VA.check_output(d_y.cpu().numpy(), by, gy, wy, "dy " + what)
    assert np.array_equal(d_in.cpu().numpy(), a_in), "the input arena was written: " + what


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("w,h", [(253, 9), (6, 5), (1, 3)])
def test_views(w, h, ch):
    """Pitched views with guards: input offsets 0..3, outputs at 8-, 4- and 2-byte alignments, tight and padded pitches, a
    gap between the frames of a batch of 3."""
    frames = _contents(w, h, ch, 77 + w)[[0, 3, 4]]
    n = len(frames)
    rb = w * ch
    with api.Context(w, h, ch, n, api.MODE_R) as ctx:
        for ks in KSIZES:
            want = D.sobel16_frames(frames, ks)
            k = 0
            for in_off in range(4):
                # outputs: (byte offset, alignment of base / pitch / frame stride) -- each of the kernel's three store forms
                for out_off, al in ((0, 8), (2, 2), (4, 4), (8, 8), (6, 2)):
                    in_al = 4 if in_off == 0 and k % 2 == 0 else 1   # 4: rows the kernel may read as dwords
                    in_pitch = VA.round_up(rb + (0, 3, 4, 13)[k % 4], in_al)
                    in_fs = VA.round_up(in_pitch * h + 5 * (k % 3), in_al)
                    pitch = VA.round_up(2 * rb + 2 * (k % 3), al)
                    fs = VA.round_up(pitch * h + 6 * (k % 4), al)
                    _run_view(ctx, frames, ks, in_pitch, in_fs, in_off, pitch, fs, out_off, seed=k, want=want)
                    k += 1


@pytest.mark.parametrize("ch", [1, 3])
def test_roi_of_a_larger_image(ch):
    """The input is an ROI whose neighbours are the parent's own pixels, the outputs ROIs of larger planes: the neighbours
    neither change a result nor are they changed."""
    w, h = 250, 70
    frames = _contents(w, h, ch, 5)[[0, 4]]
    with api.Context(w, h, ch, 2, api.MODE_O) as ctx:
        for ks in KSIZES:
            for in_off, out_off in ((0, 0), (ch * 17, 2 * ch * 9)):
                in_pitch = ch * (w + 64)
                pitch = 2 * ch * (w + 40)
                _run_view(ctx, frames, ks, in_pitch, in_pitch * (h + 3), in_off, pitch, pitch * (h + 2), out_off, fill="parent", seed=ks + 3)


def _chain(ctx, d_in, row, h, n, ks, dx, dy, out, w):
    ctx.derivatives_device(d_in.data_ptr(), row, row * h, dx.data_ptr(), dy.data_ptr(), 2 * row, 2 * row * h, n, ks)
    ctx.run_gradients_device(dx.data_ptr(), dy.data_ptr(), 2 * row, 2 * row * h, out.data_ptr(), w, w * h, n)


@pytest.mark.parametrize("piped", [False, True], ids=["plain", "pipelined"])
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("l2", [False, True], ids=["L1", "L2"])
@pytest.mark.parametrize("ks", [3, 5])
def test_chain_equals_aperture(ks, l2, ch, piped):
    """derivatives_device -> run_gradients_device gives the map HC_OPT_APERTURE 3 / 5 gives, bit for bit (no CPU reference),
    with no sync between the two calls; two such pairs back to back with rotated buffers and one sync at the end."""
    import torch
    w, h, n = 333, 130, 2
    low, high = (60, 180) if ks == 3 else (400, 1200)
    if ch == 1:
        sets = [np.stack([synth.natural(w, h, 3 + s), synth.noise(w, h, 4 + s)]) for s in (0, 10)]
    else:
        sets = [np.stack([np.stack([synth.natural(w, h, 5 + s + k), synth.noise(w, h, 6 + s + k), synth.natural(w, h, 7 + s + k)[::-1].copy()], -1)
                          for k in range(n)]) for s in (0, 10)]
    with api.Context(w, h, ch, n, api.MODE_O) as ref:
        ref.set_thresholds(low, high)
        ref.set_option(api.OPT_L2_GRADIENT, int(l2))
        ref.set_option(api.OPT_APERTURE, ks)
        want = [ref.process(s) for s in sets]
    assert any(wm.any() for wm in want)
    row = w * ch
    with api.Context(w, h, ch, n, api.MODE_O) as ctx:
        ctx.set_thresholds(low, high)
        ctx.set_option(api.OPT_L2_GRADIENT, int(l2))
        if piped:
            ctx.set_option(api.OPT_PIPELINE, 1)
        d_in = [torch.from_numpy(s).cuda() for s in sets]
        shape = sets[0].shape
        dx = [torch.full(shape, 0x5A5A, dtype=torch.int16, device="cuda") for _ in range(2)]
        dy = [torch.full(shape, 0x5A5A, dtype=torch.int16, device="cuda") for _ in range(2)]
        out = [torch.full((n, h, w), 7, dtype=torch.uint8, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        for k in range(2):
            _chain(ctx, d_in[k], row, h, n, ks, dx[k], dy[k], out[k], w)
        ctx.sync()
        for k in range(2):
            _diff(out[k].cpu().numpy(), want[k], f"chain {k} ksize {ks} l2 {l2} ch {ch} piped {piped}")
        assert ctx.last_run_info()[2] == 7


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("l2", [False, True], ids=["L1", "L2"])
@pytest.mark.parametrize("ks", [7, -1])
def test_process_aperture(ks, l2, ch):
    w, h = 301, 97
    low, high = (150, 450) if ks == 7 else (300, 900)
    frames = np.stack([synth.natural(w, h, 21), synth.noise(w, h, 22)])
    if ch == 3:
        frames = np.stack([frames, frames[::-1], np.stack([synth.noise(w, h, 23), synth.natural(w, h, 24)])], -1)
    want = np.stack([X.canny_o_from_gradients(*D.sobel16(f, ks), low, high, l2) for f in frames])
    assert want.any() and not want.all()
    with api.Context(w, h, ch, 2, api.MODE_O) as ctx:
        ctx.set_thresholds(low, high)
        ctx.set_option(api.OPT_L2_GRADIENT, int(l2))
        _diff(ctx.process_aperture(frames, ks), want, f"process_aperture ksize {ks} l2 {l2} ch {ch}")
    with api.Context(w, h, ch, 2, api.MODE_R) as ctx:
        with pytest.raises(api.HipCannyError):
            ctx.process_aperture(frames, ks)


def test_not_a_run():
    w, h = 320, 200
    frames = np.stack([synth.natural(w, h, 1), synth.noise(w, h, 2)])
    for mode in (api.MODE_O, api.MODE_R):
        with api.Context(w, h, 1, 2, mode) as ctx:
            maps = ctx.process(frames)
            info, sched, hinfo = ctx.last_run_info(), ctx.hysteresis_schedule(), ctx.hysteresis_info()
            for ks in KSIZES:
                dx, dy = ctx.derivatives(frames, ks)
                wx, wy = D.sobel16_frames(frames, ks)
                _diff(dx, wx, f"mode {mode} dx ksize {ks}")
                _diff(dy, wy, f"mode {mode} dy ksize {ks}")
            assert ctx.last_run_info() == info
            assert ctx.hysteresis_schedule() == sched
            assert ctx.hysteresis_info() == hinfo
            _diff(ctx.process(frames), maps, "the run after the derivatives")


def test_errors():
    import torch
    w, h, nb = 64, 32, 2
    with api.Context(w, h, 3, nb, api.MODE_O) as ctx:
        row = 3 * w
        d_in = torch.zeros((nb, h, row), dtype=torch.uint8, device="cuda")
        gx = torch.zeros((nb, h, row + 2), dtype=torch.int16, device="cuda")
        gy = torch.zeros((nb, h, row + 2), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        pi, px, py = d_in.data_ptr(), gx.data_ptr(), gy.data_ptr()
        ok = dict(d_in=pi, in_pitch=row, in_fs=row * h, d_dx=px, d_dy=py, pitch=2 * row + 4, fs=(2 * row + 4) * h, nframes=1, ksize=3)
        bad = [dict(d_in=0), dict(d_dx=0), dict(d_dy=0),                                   # null pointers
               dict(d_dx=px + 1), dict(d_dy=py + 1), dict(pitch=2 * row + 3), dict(fs=(2 * row + 4) * h + 1),   # odd
               dict(in_pitch=row - 1), dict(pitch=2 * row - 2),                            # rows that do not fit
               dict(ksize=0), dict(ksize=1), dict(ksize=9), dict(ksize=-3), dict(ksize=4),
               dict(nframes=0), dict(nframes=nb + 1), dict(nframes=-1),
               dict(in_pitch=1 << 31), dict(pitch=1 << 31), dict(in_pitch=(1 << 32) // h), dict(pitch=(1 << 32) // h)]   # views of 4 GiB
        for b in bad:
            with pytest.raises(api.HipCannyError) as ei:
                ctx.derivatives_device(**{**ok, **b})
            assert "hc_derivatives_device" in str(ei.value), b
        for v in (7, -1):   # the option keeps refusing what the new entry offers
            with pytest.raises(api.HipCannyError):
                ctx.set_option(api.OPT_APERTURE, v)
        ctx.derivatives_device(**{**ok, "nframes": nb, "ksize": 7})   # and the valid call runs
        ctx.sync()
        assert not gx.cpu().numpy().any() and not gy.cpu().numpy().any()   # zero frames: zero derivatives


@pytest.mark.parametrize("part", range(4))
def test_fuzz(part):
    """About 200 seeded cases in four parts: sizes up to 700 x 300, every kind, 1 / 3 channels, pitches and offsets."""
    rng = np.random.default_rng(0xD16 + part)
    for case in range(50):
        big = case % 10 == 0
        w = int(rng.integers(1, 701)) if big else int(rng.choice([rng.integers(1, 13), rng.integers(240, 260), rng.integers(1, 120)]))
        h = int(rng.integers(1, 301)) if big else int(rng.choice([rng.integers(1, 10), rng.integers(60, 70), rng.integers(1, 40)]))
        ch = int(rng.choice([1, 3]))
        n = int(rng.integers(1, 4))
        ks = int(rng.choice(KSIZES))
        kind = int(rng.integers(0, 3))
        shape = (n, h, w) if ch == 1 else (n, h, w, ch)
        if kind == 0:
            frames = rng.integers(0, 256, shape, dtype=np.uint8)
        elif kind == 1:
            frames = (rng.integers(0, 2, shape) * 255).astype(np.uint8)
        else:
            frames = np.stack([_contents(w, h, ch, int(rng.integers(1 << 30)))[4] for _ in range(n)])
        rb = w * ch
        in_pitch = rb + int(rng.choice([0, 0, 1, 2, 3, 4, 29]))
        pitch = 2 * rb + 2 * int(rng.choice([0, 0, 1, 2, 3, 16]))
        in_fs = in_pitch * h + int(rng.choice([0, 0, 1, 4, 7]))
        fs = pitch * h + 2 * int(rng.choice([0, 0, 1, 2, 5]))
        with api.Context(w, h, ch, n, api.MODE_O if case & 1 else api.MODE_R) as ctx:
            _run_view(ctx, frames, ks, in_pitch, in_fs, int(rng.integers(0, 4)), pitch, fs, 2 * int(rng.integers(0, 4)), seed=case)
