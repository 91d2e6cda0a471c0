"""hc_gaussian_blur_device (k_gauss8) on the MI355X: cv::GaussianBlur's fixed-point path for u8 frames, bit for bit against
tests/gauss_blur_ref.py (anchored by tests/test_gauss_blur_ref_cpu.py); caller views with guard bytes on both sides; the
chain blur -> hc_canny_device against canny on the reference-blurred frames run on the same context (no CPU Canny involved);
the blur keyword of canny_points / canny_auto; not a run; the refusals; a seeded fuzz."""
import os
import re

import numpy as np
import pytest

from cudacam_amd import api, synth
import gauss_blur_ref as G
import view_arena as VA

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _param(name):
    src = open(os.path.join(ROOT, "cudacam_amd", "csrc", "canny_params.h")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


STRIP_W = _param("BLUR_STRIP_W")
CHUNK_ROWS = _param("BLUR_CHUNK_ROWS")
KSIZES = G.KSIZES
BORDERS = G.BORDERS
ASYM = {3: [1, 200, 55], 5: [3, 0, 100, 120, 33], 7: [7, 9, 0, 40, 150, 0, 50]}


def _tap_sets(k):
    """sigma 0, sigma 1.4, the two one-tap shifts, one asymmetric set."""
    return [G.gaussian_taps_q8(k, 0.0), G.gaussian_taps_q8(k, 1.4), [256] + [0] * (k - 1), [0] * (k - 1) + [256], ASYM[k]]


def _contents(w, h, ch, seed):
    """Five frames: uniform random, all 0, all 255 (the 65280 edge of the 16-bit pass), a 0 / 255 checkerboard, a smoothed image."""
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
    [(1, 1), (2, 3), (3, 1), (5, 2), (7, 7), (700, 300)]
    + [(3, 5), (4, 5), (5, 5), (8, 3), (9, 4)]                                            # one lane group +- 1, two
    + [(STRIP_W - 1, 6), (STRIP_W, 6), (STRIP_W + 1, 6), (2 * STRIP_W + 1, 6)]            # strip boundaries
    + [(STRIP_W - 1, 9), (STRIP_W, 9), (STRIP_W + 1, 9), (2 * STRIP_W + 1, 9)]
    + [(11, h) for h in range(1, 9)]                                                      # heights 1 .. ksize + 1
    + [(13, CHUNK_ROWS - 1), (13, CHUNK_ROWS), (13, CHUNK_ROWS + 1), (251, 2 * CHUNK_ROWS + 1)]))   # row chunks


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_shapes(w, h, ch):
    frames = _contents(w, h, ch, 1000 * w + h)
    with api.Context(w, h, ch, len(frames), api.MODE_O) as ctx:
        for k in KSIZES:
            for taps in _tap_sets(k):
                for border in BORDERS:
                    got = ctx.gaussian_blur(frames, k, border=border, taps=taps)
                    assert got.dtype == np.uint8 and got.shape == frames.shape
                    _diff(got, G.blur_frames(frames, taps, border), f"taps {taps} border {border} {w}x{h}x{ch}")


def test_sigma_and_default_border():
    w, h = 97, 41
    frames = _contents(w, h, 1, 9)[[0, 4]]
    with api.Context(w, h, 1, 2, api.MODE_R) as ctx:
        for k in KSIZES:
            for sigma in (0.0, 0.8, 1.4, 2.0):
                _diff(ctx.gaussian_blur(frames, k, sigma), G.gauss_blur_ref(frames, k, sigma, G.REFLECT_101), f"ksize {k} sigma {sigma}")
                _diff(ctx.gaussian_blur(frames[0], k, sigma, api.BORDER_REPLICATE)[0], G.gauss_blur_ref(frames[:1], k, sigma, G.REPLICATE)[0], f"ksize {k} sigma {sigma} replicate")


def _lead(pitch):
    return VA.round_up(pitch + 64, 16)   # the view's alignment is that of its base offset


def _run_view(ctx, frames, taps, border, in_pitch, in_fs, in_off, pitch, fs, out_off, fill="random", seed=0, want=None):
    """One call on guarded arenas: the output view must hold the reference, every other byte of both arenas must be unchanged."""
    import torch
    n, h, w = frames.shape[:3]
    ch = 1 if frames.ndim == 3 else 3
    a_in, off_in = VA.make_input(frames, in_pitch, in_fs, in_off, fill, lead=_lead(in_pitch), seed=seed)
    b_out, g_out = VA.make_output(n, h, ch * w, pitch, fs, out_off, lead=_lead(pitch), seed=seed + 1)
    d_in, d_out = (torch.from_numpy(v).cuda() for v in (a_in, b_out))
    torch.cuda.synchronize()
    ctx.gaussian_blur_device(d_in.data_ptr() + off_in, in_pitch, in_fs if in_fs else in_pitch * h, d_out.data_ptr() + g_out.offset,
                             pitch, fs if fs else pitch * h, n, len(taps), taps, border)
    ctx.sync()
    want = want if want is not None else G.blur_frames(frames, taps, border)
    what = f"taps {taps} border {border} {w}x{h}x{ch} in(pitch {in_pitch}, off {in_off}) out(pitch {pitch}, off {out_off})"
    VA.check_output(d_out.cpu().numpy(), b_out, g_out, want, what)
    assert np.array_equal(d_in.cpu().numpy(), a_in), "the input arena was written: " + what


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("w,h", [(253, 9), (6, 5), (1, 3)])
def test_views(w, h, ch):
    """Pitched views with guards: input offsets 0..3, output offsets 0..3, tight and padded pitches, 4-aligned views (dword
    loads / stores) and others, a gap between the frames of a batch of 3."""
    frames = _contents(w, h, ch, 77 + w)[[0, 3, 4]]
    n = len(frames)
    rb = w * ch
    with api.Context(w, h, ch, n, api.MODE_R) as ctx:
        for k in KSIZES:
            for taps, border in ((G.gaussian_taps_q8(k, 1.4), G.REFLECT_101), (ASYM[k], G.REPLICATE)):
                want = G.blur_frames(frames, taps, border)
                c = 0
                for in_off in range(4):
                    for out_off in range(4):
                        in_al = 4 if in_off == 0 and c % 2 == 0 else 1    # 4: rows the kernel may read as dwords
                        out_al = 4 if out_off == 0 and c % 4 < 2 else 1   # 4: rows it may write as dwords
                        in_pitch = VA.round_up(rb + (0, 3, 4, 13)[c % 4], in_al)
                        in_fs = VA.round_up(in_pitch * h + 5 * (c % 3), in_al)
                        pitch = VA.round_up(rb + (0, 5, 8, 1)[(c // 2) % 4], out_al)
                        fs = VA.round_up(pitch * h + 3 * (c % 4), out_al)
                        _run_view(ctx, frames, taps, border, in_pitch, in_fs, in_off, pitch, fs, out_off, seed=c, want=want)
                        c += 1


@pytest.mark.parametrize("ch", [1, 3])
def test_roi_of_a_larger_image(ch):
    """The input is an ROI whose neighbours are the parent's own pixels on both sides, the output an ROI of a larger image: the
    neighbours neither change a result (the border is made of the ROI's own pixels) nor are they changed."""
    w, h = 250, 70
    frames = _contents(w, h, ch, 5)[[0, 4]]
    with api.Context(w, h, ch, 2, api.MODE_O) as ctx:
        for k in KSIZES:
            for border in BORDERS:
                for in_off, out_off in ((0, 0), (ch * 17, ch * 9)):
                    in_pitch = ch * (w + 64)
                    pitch = ch * (w + 40)
                    _run_view(ctx, frames, G.gaussian_taps_q8(k, 1.4), border, in_pitch, in_pitch * (h + 3), in_off, pitch, pitch * (h + 2), out_off,
                              fill="parent", seed=k + 3)


def _frames_for_chain(w, h, ch, n):
    if ch == 1:
        return [np.stack([synth.natural(w, h, 3 + s), synth.noise(w, h, 4 + s)]) for s in (0, 10)]
    return [np.stack([np.stack([synth.natural(w, h, 5 + s + k), synth.noise(w, h, 6 + s + k), synth.natural(w, h, 7 + s + k)[::-1].copy()], -1)
                      for k in range(n)]) for s in (0, 10)]


@pytest.mark.parametrize("piped", [False, True], ids=["plain", "pipelined"])
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("aperture", [3, 7])
def test_blur_canny_chain(aperture, ch, piped):
    """blur_canny(frames, 5, 1.4, ...) equals canny on the reference-blurred frames, run on the same context; then two pairs
    gaussian_blur_device -> canny_device back to back with rotated buffers and one sync at the end."""
    import torch
    w, h, n = 333, 130, 2
    low, high = (40, 120) if aperture == 3 else (1500, 4500)
    sets = _frames_for_chain(w, h, ch, n)
    taps = G.gaussian_taps_q8(5, 1.4)
    row = w * ch
    with api.Context(w, h, ch, n, api.MODE_O) as ctx:
        if piped:
            ctx.set_option(api.OPT_PIPELINE, 1)
        want = [ctx.canny(G.gauss_blur_ref(s, 5, 1.4), low, high, aperture) for s in sets]
        for wm in want:
            assert wm.any() and not wm.all()
        for s, wm in zip(sets, want):
            _diff(ctx.blur_canny(s, 5, 1.4, low, high, aperture), wm, f"blur_canny aperture {aperture} ch {ch} piped {piped}")
        d_in = [torch.from_numpy(s).cuda() for s in sets]
        tmp = [torch.full(sets[0].shape, 0x5A, dtype=torch.uint8, device="cuda") for _ in range(2)]
        out = [torch.full((n, h, w), 7, dtype=torch.uint8, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        for k in range(2):
            ctx.gaussian_blur_device(d_in[k].data_ptr(), row, row * h, tmp[k].data_ptr(), row, row * h, n, 5, taps)
            ctx.canny_device(tmp[k].data_ptr(), row, row * h, out[k].data_ptr(), w, w * h, n, low, high, aperture)
        ctx.sync()
        for k in range(2):
            _diff(tmp[k].cpu().numpy(), G.gauss_blur_ref(sets[k], 5, 1.4), f"chain {k}: the blurred frames")
            _diff(out[k].cpu().numpy(), want[k], f"chain {k} aperture {aperture} ch {ch} piped {piped}")
    with api.Context(w, h, ch, n, api.MODE_R) as ctx:
        with pytest.raises(api.HipCannyError):
            ctx.blur_canny(sets[0], 5, 1.4, low, high, aperture)


@pytest.mark.parametrize("ch", [1, 3])
def test_blur_keyword_of_points_and_auto(ch):
    w, h, n = 333, 130, 2
    frames = _frames_for_chain(w, h, ch, n)[0]
    for blur in ((3, 0.0), (5, 1.4)):
        ref = G.gauss_blur_ref(frames, *blur)
        with api.Context(w, h, ch, n, api.MODE_O) as ctx:
            maps, counts, lists = ctx.canny_points(frames, 40, 120, blur=blur)
            wmaps, wcounts, wlists = ctx.canny_points(ref, 40, 120)
            assert wmaps.any() and not wmaps.all()
            _diff(maps, wmaps, f"canny_points blur {blur}")
            assert np.array_equal(counts, wcounts) and all(np.array_equal(a, b) for a, b in zip(lists, wlists))
            for rule in ("median", "otsu"):
                amaps, thr = ctx.canny_auto(frames, rule, blur=blur)
                wamaps, wthr = ctx.canny_auto(ref, rule)
                assert np.array_equal(thr, wthr), (rule, thr, wthr)
                _diff(amaps, wamaps, f"canny_auto {rule} blur {blur}")


def test_not_a_run():
    w, h = 320, 200
    frames = np.stack([synth.natural(w, h, 1), synth.noise(w, h, 2)])
    for mode in (api.MODE_O, api.MODE_R):
        with api.Context(w, h, 1, 2, mode) as ctx:
            maps = ctx.process(frames)
            info, sched, hinfo = ctx.last_run_info(), ctx.hysteresis_schedule(), ctx.hysteresis_info()
            for k in KSIZES:
                for border in BORDERS:
                    _diff(ctx.gaussian_blur(frames, k, 1.4, border), G.gauss_blur_ref(frames, k, 1.4, border), f"mode {mode} ksize {k} border {border}")
            assert ctx.last_run_info() == info
            assert ctx.hysteresis_schedule() == sched
            assert ctx.hysteresis_info() == hinfo
            _diff(ctx.process(frames), maps, "the run after the blur")


def test_errors():
    import torch
    w, h, nb = 64, 32, 2
    with api.Context(w, h, 3, nb, api.MODE_O) as ctx:
        row = 3 * w
        pitch = row + 4
        d_in = torch.zeros((nb, h, row), dtype=torch.uint8, device="cuda")
        d_out = torch.full((nb + 1, h, pitch), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        pi, po = d_in.data_ptr(), d_out.data_ptr()
        ok = dict(d_in=pi, in_pitch=row, in_fs=row * h, d_out=po, out_pitch=pitch, out_fs=pitch * h, nframes=1, ksize=3, taps=[64, 128, 64])
        bad = [dict(d_in=0), dict(d_out=0),                                                # null pointers
               dict(ksize=0, taps=[]), dict(ksize=1, taps=[256]), dict(ksize=4, taps=[64, 64, 64, 64]), dict(ksize=9, taps=[0] * 4 + [256] + [0] * 4),
               dict(ksize=-1, taps=[64, 128, 64]),
               dict(border=2), dict(border=-1), dict(border=4),
               dict(taps=[257, 0, 0]), dict(taps=[0, 300, 0]), dict(taps=[64, 127, 64]), dict(taps=[64, 129, 64]), dict(taps=[0, 0, 0]),
               dict(taps=[65535, 1, 256]),
               dict(in_pitch=row - 1), dict(out_pitch=row - 1),                            # rows that do not fit
               dict(nframes=0), dict(nframes=nb + 1), dict(nframes=-1),
               dict(nframes=2, in_fs=row * h - 1), dict(nframes=2, out_fs=pitch * h - 1),
               dict(in_pitch=1 << 31), dict(out_pitch=1 << 31), dict(in_pitch=(1 << 32) // h), dict(out_pitch=(1 << 32) // h),   # views of 4 GiB
               dict(d_out=pi, out_pitch=row, out_fs=row * h),                              # in place
               dict(d_out=pi + row * (h - 1) + row - 1, out_pitch=row, out_fs=row * h),    # one shared byte
               dict(d_in=po + 1, in_pitch=pitch, in_fs=pitch * h),
               dict(nframes=2, d_in=po + pitch * h, in_pitch=pitch, in_fs=pitch * h)]      # frame 0 of the input is frame 1 of the output
        for b in bad:
            with pytest.raises(api.HipCannyError) as ei:
                ctx.gaussian_blur_device(**{**ok, **b})
            assert "hc_gaussian_blur_device" in str(ei.value), b
        before = d_out.cpu().numpy()
        assert (before == 9).all()                                                         # no refused call wrote anything
        # neighbours that touch -- the input begins where the output view ends -- are fine, and the valid call runs
        d_both = torch.zeros(2 * row * h, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        pb = d_both.data_ptr()
        ctx.gaussian_blur_device(pb + row * h, row, row * h, pb, row, row * h, 1, 7, G.gaussian_taps_q8(7, 2.0))
        ctx.gaussian_blur_device(**{**ok, "nframes": nb, "ksize": 5, "taps": [16, 64, 96, 64, 16], "border": api.BORDER_REPLICATE})
        ctx.sync()
        after = d_out.cpu().numpy()
        assert not after[:nb, :, :row].any() and (after[:nb, :, row:] == 9).all() and (after[nb] == 9).all()   # zero frames: zero blur


@pytest.mark.parametrize("part", range(4))
def test_fuzz(part):
    """About 200 seeded cases in four parts: sizes up to 700 x 300, any ksize, border, channels, taps, pitches and offsets."""
    rng = np.random.default_rng(0xB1A + part)
    for case in range(50):
        big = case % 10 == 0
        w = int(rng.integers(1, 701)) if big else int(rng.choice([rng.integers(1, 13), rng.integers(240, 260), rng.integers(1, 120)]))
        h = int(rng.integers(1, 301)) if big else int(rng.choice([rng.integers(1, 10), rng.integers(60, 70), rng.integers(1, 40)]))
        ch = int(rng.choice([1, 3]))
        n = int(rng.integers(1, 4))
        k = int(rng.choice(KSIZES))
        border = int(rng.choice(BORDERS))
        tk = int(rng.integers(0, 3))
        if tk == 0:
            taps = G.gaussian_taps_q8(k, float(rng.uniform(0.0, 3.0)))
        elif tk == 1:   # any split of 256 over k taps
            cuts = np.sort(rng.integers(0, 257, k - 1))
            taps = [int(v) for v in np.diff(np.concatenate([[0], cuts, [256]]))]
        else:
            taps = [0] * k
            taps[int(rng.integers(0, k))] = 256
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
        pitch = rb + int(rng.choice([0, 0, 1, 2, 3, 4, 16]))
        in_fs = in_pitch * h + int(rng.choice([0, 0, 1, 4, 7]))
        fs = pitch * h + int(rng.choice([0, 0, 1, 4, 5]))
        with api.Context(w, h, ch, n, api.MODE_O if case & 1 else api.MODE_R) as ctx:
            _run_view(ctx, frames, taps, border, in_pitch, in_fs, int(rng.integers(0, 4)), pitch, fs, int(rng.integers(0, 4)), seed=case)
