"""hc_morphology_device (k_morph8) on the MI355X: cv::erode / cv::dilate / cv::morphologyEx (open, close, gradient) for u8
frames, value for value against tests/morph_ref.py (anchored by tests/test_morph_ref_cpu.py); caller views with guard bytes on
both sides; the passes of OPEN / CLOSE under a small scratch bound; the frame limits; the chain canny -> close -> components,
also behind pipelined runs; not a run; the wrapper's iterations; the refusals; a seeded fuzz."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cudacam_amd import api, synth
import morph_ref as M
import view_arena as VA

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _param(name):
    src = open(os.path.join(ROOT, "cudacam_amd", "csrc", "canny_params.h")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


STRIP_W = _param("BLUR_STRIP_W")
CHUNK_ROWS = _param("BLUR_CHUNK_ROWS")
FUZZ_SEED = 20261020


def _elements(k):
    """RECT, CROSS, ELLIPSE, [K/2, 0, .., -1] (asymmetric with an empty row), the centre pixel alone (identity), the top row alone
    (windows wholly outside the frame at row 0), and one that uses every half-width."""
    r = k // 2
    asym = [r] + [0] * (k - 2) + [-1]
    centre = [0 if j == r else -1 for j in range(k)]
    top = [r] + [-1] * (k - 1)
    every = [(j % (r + 1)) for j in range(k)]
    return [M.structuring_spans(s, k) for s in M.SHAPES] + [asym, centre, top, every]


def _contents(w, h, ch, seed):
    """Random u8, all 0, all 255, a 0 / 255 checkerboard, impulses at the four corners and the centre, a sparse 0 / 255 map."""
    rng = np.random.default_rng(seed)
    shape = (h, w) if ch == 1 else (h, w, ch)
    rnd = rng.integers(0, 256, shape, dtype=np.uint8)
    cb = ((np.add.outer(np.arange(h), np.arange(w)) & 1) * 255).astype(np.uint8)
    imp = np.zeros((h, w), np.uint8)
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2)):
        imp[y, x] = 255
    sparse = ((rng.random((h, w)) < 0.01) * 255).astype(np.uint8)
    if ch == 3:
        cb = np.stack([cb, 255 - cb, cb], -1)
        imp = np.stack([imp, 255 - imp, imp], -1)
        sparse = np.stack([sparse, np.roll(sparse, 1, 0), 255 - sparse], -1)
    return np.stack([rnd, np.zeros(shape, np.uint8), np.full(shape, 255, np.uint8), cb, imp, sparse])


def _diff(got, want, what):
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    first = [(tuple(int(v) for v in p), int(got[tuple(p)]), int(want[tuple(p)])) for p in bad[:8]]
    raise AssertionError(f"{what}: {len(bad)} of {got.size} differ; first (pos, hip, ref): {first}")


SHAPES = sorted(set(
    [(1, 1), (2, 3), (3, 1), (5, 2), (7, 7)]
    + [(3, 5), (4, 5), (5, 5), (8, 3), (9, 4)]                                            # one lane group +- 1, two
    + [(STRIP_W - 1, 6), (STRIP_W, 6), (STRIP_W + 1, 6), (2 * STRIP_W + 1, 9)]            # strip boundaries
    + [(11, h) for h in range(1, 9)]                                                      # heights 1 .. ksize + 1
    + [(13, CHUNK_ROWS - 1), (13, CHUNK_ROWS), (13, CHUNK_ROWS + 1), (251, 2 * CHUNK_ROWS + 1)]))   # row chunks


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_shapes(w, h, ch):
    frames = _contents(w, h, ch, 1000 * w + h)
    with api.Context(w, h, ch, len(frames), api.MODE_O) as ctx:
        for k in M.KSIZES:
            for spans in _elements(k):
                ref = {M.DILATE: M.dilate(frames, spans), M.ERODE: M.erode(frames, spans)}
                ref[M.OPEN], ref[M.CLOSE] = M.dilate(ref[M.ERODE], spans), M.erode(ref[M.DILATE], spans)
                ref[M.GRADIENT] = M.morph(frames, M.GRADIENT, spans)
                for op in M.OPS:
                    got = ctx.morphology(frames, op, ksize=k, spans=spans)
                    assert got.dtype == np.uint8 and got.shape == frames.shape
                    _diff(got, ref[op], f"op {op} spans {spans} {w}x{h}x{ch}")


def test_one_channel_maps_on_a_three_channel_context():
    """`channels` is the caller's: edge maps are one-channel on every context."""
    w, h = 37, 21
    maps = _contents(w, h, 1, 4)
    with api.Context(w, h, 3, len(maps), api.MODE_O) as ctx:
        for shape in M.SHAPES:
            _diff(ctx.morphology(maps, api.MORPH_CLOSE, shape, 5), M.morph(maps, M.CLOSE, M.structuring_spans(shape, 5)), f"shape {shape}")


def _lead(pitch):
    return VA.round_up(pitch + 64, 16)   # the view's alignment is that of its base offset


def _run_view(ctx, frames, op, spans, in_pitch, in_fs, in_off, pitch, fs, out_off, seed, want):
    """One call on guarded arenas: the output view must hold the reference, every other byte of both arenas must be unchanged."""
    import torch
    n, h, w = frames.shape[:3]
    ch = 1 if frames.ndim == 3 else 3
    a_in, off_in = VA.make_input(frames, in_pitch, in_fs, in_off, "random", lead=_lead(in_pitch), seed=seed)
    b_out, g_out = VA.make_output(n, h, ch * w, pitch, fs, out_off, lead=_lead(pitch), seed=seed + 1)
    d_in, d_out = (torch.from_numpy(v).cuda() for v in (a_in, b_out))
    torch.cuda.synchronize()
    ctx.morphology_device(d_in.data_ptr() + off_in, in_pitch, in_fs, d_out.data_ptr() + g_out.offset, pitch, fs, n, ch, op, len(spans), spans)
    ctx.sync()
    what = f"op {op} spans {spans} {w}x{h}x{ch} in(pitch {in_pitch}, off {in_off}) out(pitch {pitch}, off {out_off})"
    VA.check_output(d_out.cpu().numpy(), b_out, g_out, want, what)
    assert np.array_equal(d_in.cpu().numpy(), a_in), "the input arena was written: " + what


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("w,h", [(253, 9), (6, 5), (1, 3)])
def test_views(w, h, ch):
    """Pitched views with guards: input offsets 0..3, output offsets 0..3, tight and padded pitches, 4-aligned views (dword loads
    / stores) and others, a gap between the frames of a batch of 3 -- for every op, OPEN / CLOSE (whose scratch pitch differs from
    both views') included."""
    frames = _contents(w, h, ch, 77 + w)[[0, 3, 5]]
    rb = w * ch
    with api.Context(w, h, ch, 3, api.MODE_R) as ctx:
        c = 0
        for k in M.KSIZES:
            spans = _elements(k)[(2, 3, 6)[k // 2 - 1]]
            for op in M.OPS:
                want = M.morph(frames, op, spans)
                for in_off in range(4):
                    for out_off in range(4):
                        in_al = 4 if in_off == 0 and c % 2 == 0 else 1    # 4: rows the kernel may read as dwords
                        out_al = 4 if out_off == 0 and c % 4 < 2 else 1   # 4: rows it may write as dwords
                        in_pitch = VA.round_up(rb + (0, 3, 4, 13)[c % 4], in_al)
                        in_fs = VA.round_up(in_pitch * h + 5 * (c % 3), in_al)
                        pitch = VA.round_up(rb + (0, 5, 8, 1)[(c // 2) % 4], out_al)
                        fs = VA.round_up(pitch * h + 3 * (c % 4), out_al)
                        _run_view(ctx, frames, op, spans, in_pitch, in_fs, in_off, pitch, fs, out_off, c, want)
                        c += 1


def test_passes_under_a_small_scratch_bound():
    """4 frames of CLOSE in 4, 2 and 1 passes give identical results; a bound below one frame is refused."""
    w, h, ch = 61, 9, 3
    frames = _contents(w, h, ch, 8)[[0, 3, 4, 5]]
    spans = M.structuring_spans(M.ELLIPSE, 5)
    want = M.morph(frames, M.CLOSE, spans)
    frame = VA.round_up(w * ch, 4) * h
    with api.Context(w, h, ch, 4, api.MODE_O) as ctx:
        for bound in (frame, 2 * frame - 1, 2 * frame, 3 * frame, 4 * frame - 1, 4 * frame, 0):   # 4, 4, 2, 2, 2, 1 passes; 0: the default
            ctx.set_option(api.OPT_TEST_HOUGH_SCRATCH, bound)
            _diff(ctx.morphology(frames, api.MORPH_CLOSE, ksize=5, spans=spans), want, f"bound {bound}")
            _diff(ctx.morphology(frames, api.MORPH_OPEN, ksize=5, spans=spans), M.morph(frames, M.OPEN, spans), f"open, bound {bound}")
        ctx.set_option(api.OPT_TEST_HOUGH_SCRATCH, frame - 1)
        with pytest.raises(api.HipCannyError, match="hc_morphology_device: one frame of intermediate results exceeds"):
            ctx.morphology(frames, api.MORPH_CLOSE, ksize=5, spans=spans)
        _diff(ctx.morphology(frames, api.MORPH_GRADIENT, ksize=5, spans=spans), M.morph(frames, M.GRADIENT, spans), "gradient needs no scratch")


def test_frame_limits_on_a_per_channel_context():
    """A per-channel context accepts 3 * max_batch one-channel maps and refuses one more; 3-channel frames stop at max_batch."""
    import torch
    w, h, mb = 19, 7, 2
    maps = np.random.default_rng(3).integers(0, 256, (3 * mb + 1, h, w), dtype=np.uint8)
    with api.Context(w, h, 3, mb, api.MODE_O) as ctx:
        ctx.set_option(api.OPT_PER_CHANNEL, 1)
        _diff(ctx.morphology(maps[:3 * mb], api.MORPH_DILATE), M.dilate(maps[:3 * mb], [1, 1, 1]), "3 * max_batch maps")
        with pytest.raises(api.HipCannyError, match="hc_morphology_device: nframes out of range"):
            ctx.morphology(maps, api.MORPH_DILATE)
        bgr = np.random.default_rng(4).integers(0, 256, (mb + 1, h, w, 3), dtype=np.uint8)
        _diff(ctx.morphology(bgr[:mb], api.MORPH_ERODE), M.erode(bgr[:mb], [1, 1, 1]), "max_batch frames")
        with pytest.raises(api.HipCannyError, match="hc_morphology_device: nframes out of range"):
            ctx.morphology(bgr, api.MORPH_ERODE)


def _scene(w, h, n, seed):
    return np.stack([synth.natural(w, h, seed + i) for i in range(n)])


def test_canny_components_with_close():
    """canny_components(close=(MORPH_RECT, 3)) against canny_device -> morph_ref close on the host -> connected_components, all
    on the same context; with close=None the method does what it did."""
    import torch
    w, h, n = 320, 200, 3
    frames = _scene(w, h, n, 40)
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        plain = ctx.canny_components(frames, 60, 150)
        src = torch.from_numpy(frames).cuda()
        out = torch.empty_like(src)
        torch.cuda.synchronize()
        ctx.canny_device(src.data_ptr(), w, w * h, out.data_ptr(), w, w * h, n, 60, 150)
        ctx.sync()
        edges = out.cpu().numpy()
        assert np.array_equal(plain[0], edges)
        closed = M.morph(edges, M.CLOSE, [1, 1, 1])
        want = ctx.connected_components(closed)
        got = ctx.canny_components(frames, 60, 150, close=(api.MORPH_RECT, 3))
        _diff(got[0], closed, "the closed maps")
        assert np.array_equal(got[1], want[0]) and np.array_equal(got[2], want[1])
        for f in range(n):
            assert np.array_equal(got[3][f], want[2][f]) and np.array_equal(got[4][f], want[3][f])
        assert (got[2] <= plain[2]).all() and (got[2] < plain[2]).any()   # closing joins broken contours


def test_behind_pipelined_runs_and_not_a_run():
    """The entry reads the output of pipelined runs still in flight (it must complete them first), and it is not a run:
    hc_last_run_info and the schedule words are unchanged across a call."""
    import torch
    w, h, n = 256, 128, 2
    sets = [_scene(w, h, n, 70 + 10 * i) for i in range(3)]
    spans = M.structuring_spans(M.CROSS, 3)
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        ctx.set_thresholds(40, 90)
        ctx.set_option(api.OPT_PIPELINE, 1)
        srcs = [torch.from_numpy(s).cuda() for s in sets]
        outs = [torch.empty_like(s) for s in srcs]
        dsts = [torch.empty_like(s) for s in srcs]
        torch.cuda.synchronize()
        for s, o in zip(srcs, outs):
            ctx.run_device(s.data_ptr(), w, w * h, o.data_ptr(), w, w * h, n)
        for o, d in zip(outs, dsts):
            ctx.morphology_device(o.data_ptr(), w, w * h, d.data_ptr(), w, w * h, n, 1, api.MORPH_CLOSE, 3, spans)
        ctx.sync()
        for o, d in zip(outs, dsts):
            edges = o.cpu().numpy()
            assert edges.any()
            _diff(d.cpu().numpy(), M.morph(edges, M.CLOSE, spans), "behind a pipelined run")
        info = (C.c_int * len(api.SCHEDULE_FIELDS))()
        ri = [C.c_int(-5) for _ in range(3)]

        def state():
            assert ctx.lib.hc_last_hysteresis_schedule(ctx.handle, info, len(info)) >= 0
            assert ctx.lib.hc_last_run_info(ctx.handle, *[C.byref(v) for v in ri]) == 0
            return list(info), [v.value for v in ri], ctx.hysteresis_info()
        before = state()
        ctx.morphology_device(outs[0].data_ptr(), w, w * h, dsts[1].data_ptr(), w, w * h, n, 1, api.MORPH_GRADIENT, 3, spans)
        ctx.sync()
        assert state() == before
        _diff(dsts[1].cpu().numpy(), M.morph(outs[0].cpu().numpy(), M.GRADIENT, spans), "after the state check")


@pytest.mark.parametrize("ch", [1, 3])
def test_wrapper_iterations(ch):
    w, h = 45, 23
    frames = _contents(w, h, ch, 12)[[0, 3, 5]]
    with api.Context(w, h, ch, 3, api.MODE_O) as ctx:
        for shape, k in ((api.MORPH_RECT, 3), (api.MORPH_ELLIPSE, 5)):
            spans = M.structuring_spans(shape, k)
            for op in M.OPS:
                for it in (1, 2, 3):
                    _diff(ctx.morphology(frames, op, shape, k, iterations=it), M.morph_iterated(frames, op, spans, it), f"op {op} shape {shape} ksize {k} x{it}")
        import torch
        t = torch.from_numpy(frames).cuda()
        _diff(ctx.morphology(t, api.MORPH_DILATE), M.dilate(frames, [1, 1, 1]), "a torch tensor in")
        _diff(ctx.morphology(frames[0], api.MORPH_ERODE)[0], M.erode(frames[:1], [1, 1, 1])[0], "one frame in")


def test_refusals():
    """Every refusal through the C entry, with the entry's name in hc_last_error; the following valid call is still correct."""
    import torch
    w, h, n = 33, 12, 2
    frames = np.random.default_rng(6).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    row = 3 * w
    fs = row * h
    with api.Context(w, h, 3, n, api.MODE_O) as ctx, api.Context(w, h, 1, n, api.MODE_O) as mono:
        src = torch.from_numpy(frames).cuda()
        guard = np.full((n, h, w, 3), 93, np.uint8)
        dst = torch.from_numpy(guard).cuda()
        torch.cuda.synchronize()
        L, H_ = ctx.lib, ctx.handle
        R3 = (C.c_int8 * 3)(1, 1, 1)

        def call(handle=H_, d_in=src.data_ptr(), ip=row, ifs=fs, d_out=dst.data_ptr(), op_=row, ofs=fs, nf=n, ch=3, op=1, k=3, spans=R3):
            return L.hc_morphology_device(handle, C.c_void_p(d_in), ip, ifs, C.c_void_p(d_out), op_, ofs, nf, ch, op, k, spans)
        bad = [
            ("null", dict(d_in=None)), ("null", dict(d_out=None)), ("null", dict(spans=None)), ("null", dict(handle=None)),
            ("channels must be 1 or 3", dict(ch=2)), ("channels must be 1 or 3", dict(ch=0)),
            ("3-channel context", dict(handle=mono.handle)),
            ("op must be", dict(op=5)), ("op must be", dict(op=-1)),
            ("ksize 3, 5 or 7", dict(k=4)), ("ksize 3, 5 or 7", dict(k=9)),
            ("span outside", dict(spans=(C.c_int8 * 3)(1, 2, 1))), ("span outside", dict(spans=(C.c_int8 * 3)(1, -2, 1))),
            ("empty", dict(spans=(C.c_int8 * 3)(-1, -1, -1))),
            ("pitch smaller than a row", dict(ip=row - 1)), ("pitch smaller than a row", dict(op_=row - 1)),
            ("nframes out of range", dict(nf=0)), ("nframes out of range", dict(nf=n + 1)),
            ("frame stride below", dict(ifs=fs - 1)), ("frame stride below", dict(ofs=fs - 1)),
            ("2^32", dict(ip=(1 << 32) // h + 1, ifs=((1 << 32) // h + 1) * h, nf=1)),
            ("overlap", dict(d_out=src.data_ptr())), ("overlap", dict(d_out=src.data_ptr() + n * fs - 1)),
        ]
        for text, kw in bad:
            assert call(**kw) == -1, (text, kw)
            err = L.hc_last_error().decode()
            assert err.startswith("hc_morphology_device: ") and text in err, (text, err)
        ctx.sync()
        assert np.array_equal(dst.cpu().numpy(), guard), "a refused call wrote"
        assert call() == 0
        ctx.sync()
        _diff(dst.cpu().numpy(), M.dilate(frames, [1, 1, 1]), "the valid call after the refusals")
        # views that touch are fine
        both = torch.empty(2 * n * fs, dtype=torch.uint8, device="cuda")
        both[:n * fs] = src.reshape(-1)
        torch.cuda.synchronize()
        assert call(d_in=both.data_ptr(), d_out=both.data_ptr() + n * fs) == 0
        ctx.sync()
        _diff(both[n * fs:].cpu().numpy().reshape(frames.shape), M.dilate(frames, [1, 1, 1]), "touching views")


def test_fuzz():
    """Seeded: a few hundred small random (shape, op, spans, view) cases, grouped by frame size so that a context serves several."""
    import torch
    rng = np.random.default_rng(FUZZ_SEED)
    case = 0
    try:
        for _ in range(40):
            w = int(rng.choice([1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 247, 248, 249, 300]))
            h = int(rng.integers(1, 70)) if rng.random() < 0.3 else int(rng.integers(1, 12))
            ch = int(rng.choice([1, 3]))
            n = int(rng.integers(1, 4))
            with api.Context(w, h, ch, n, api.MODE_O) as ctx:
                for _ in range(8):
                    case += 1
                    k = int(rng.choice(M.KSIZES))
                    spans = [int(v) for v in rng.integers(-1, k // 2 + 1, k)]
                    if all(s < 0 for s in spans):
                        spans[int(rng.integers(0, k))] = 0
                    op = int(rng.choice(M.OPS))
                    shape = (n, h, w) if ch == 1 else (n, h, w, ch)
                    frames = rng.integers(0, 256, shape, dtype=np.uint8) if rng.random() < 0.6 else ((rng.random(shape) < 0.1) * 255).astype(np.uint8)
                    rb = w * ch
                    in_off, out_off = int(rng.integers(0, 4)), int(rng.integers(0, 4))
                    in_pitch, pitch = rb + int(rng.integers(0, 9)), rb + int(rng.integers(0, 9))
                    in_fs, fs = in_pitch * h + int(rng.integers(0, 7)), pitch * h + int(rng.integers(0, 7))
                    _run_view(ctx, frames, op, spans, in_pitch, in_fs, in_off, pitch, fs, out_off, case, M.morph(frames, op, spans))
    except BaseException:
        print(f"test_fuzz: seed {FUZZ_SEED}, case {case}")
        raise
