"""hc_histogram_device (k_hist256) and hc_auto_thresholds_device (k_auto_thr) on the MI355X: exact against np.bincount /
tests/auto_thr_ref.py.  The shapes are the smallest at which the kernel's paths differ: rows shorter than a dword, rows with
a ragged head and tail at every base offset, rows longer than one trip of the four-dwords-in-flight loop (1024 bytes), frames
lower and higher than the 8-row chunk a small batch gets, and one 1920 x 1080 x 3 frame at the 64-row chunk."""
import numpy as np
import pytest

import auto_thr_ref as R
import view_arena as VA
from cudacam_amd import api, synth

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 5, 61, 64, 250, 257)
HEIGHTS = (1, 2, 65, 200)   # the chunk of these batches is 8 rows: 65 and 200 span several work items per frame


def _content(kind, w, h, ch, seed):
    def one(k):
        if kind == "flat0":
            return synth.flat(w, h, 0)
        if kind == "flat255":
            return synth.flat(w, h, 255)
        if kind == "noise":
            return synth.noise(w, h, seed + k)
        if kind == "natural":
            return synth.natural(w, h, seed + k)
        rows = np.where(np.arange(h)[:, None] % 2 == 0, 17, 200).astype(np.uint8)   # rows alternate two values
        return np.ascontiguousarray(np.broadcast_to(rows, (h, w)))
    return one(0) if ch == 1 else np.stack([one(0), one(1), one(2)], -1)


def _want(frames):
    return np.stack([np.bincount(f.reshape(-1), minlength=256) for f in frames]).astype(np.uint32)


def _hist_view(ctx, frames, pitch, frame_stride=None, base_off=0, fill="random", seed=0):
    """The histograms of `frames` placed at pitch / frame stride / base offset in a guarded arena; the arena is unchanged."""
    import torch
    n, h = frames.shape[:2]
    arena, off = VA.make_input(frames, pitch, frame_stride, base_off, fill, seed=seed)
    g = VA.input_geometry(frames, pitch, frame_stride, base_off)
    d = torch.from_numpy(arena).cuda()
    hist = torch.full((n, 256), -1, dtype=torch.int32, device="cuda")   # the entry zeroes the table itself
    torch.cuda.synchronize()
    ctx.histogram_device(d.data_ptr() + off, pitch, g.frame_stride, n, hist.data_ptr())
    ctx.sync()
    assert np.array_equal(d.cpu().numpy(), arena), "the input arena was written"
    return hist.cpu().numpy().view(np.uint32)


def _same(got, frames, what):
    want = _want(frames)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} bins differ; first (frame, bin, hip, numpy): "
                             f"{[(int(f), int(b), int(got[f, b]), int(want[f, b])) for f, b in bad[:8]]}")


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("w", WIDTHS)
def test_every_width_height_layout(w, ch):
    rb = w * ch
    for h in HEIGHTS:
        for n in (1, 3):
            frames = np.stack([_content("noise" if k % 2 else "natural", w, h, ch, 10 * w + h + k) for k in range(n)])
            with api.Context(w, h, ch, 3, api.MODE_O if (w + h) % 2 else api.MODE_R) as ctx:   # either mode
                assert ctx.hysteresis_schedule()["launches"] == 0
                _same(ctx.histogram(frames), frames, f"Context.histogram {w}x{h}x{ch} n={n}")
                _same(_hist_view(ctx, frames, rb), frames, f"tight {w}x{h}x{ch} n={n}")
                # pitched rows, padding poisoned with 0xFF (never counted); a gap between the frames
                _same(_hist_view(ctx, frames, VA.round_up(rb, 4) + 8, (VA.round_up(rb, 4) + 8) * h + 12, fill="ff"), frames, f"pitched {w}x{h}x{ch} n={n}")
                for off in (1, 2, 3):   # the bytewise head and tail: base offsets, odd pitches
                    _same(_hist_view(ctx, frames, rb + 3, (rb + 3) * h + 5, base_off=off, seed=off), frames, f"offset {off} {w}x{h}x{ch} n={n}")
                # an ROI of a larger natural image: the neighbours are pixels of the parent
                _same(_hist_view(ctx, frames, rb + 37, base_off=11, fill="parent"), frames, f"ROI {w}x{h}x{ch} n={n}")
                assert ctx.hysteresis_schedule()["launches"] == 0   # not a run: nothing of the runs' diagnostics moved


@pytest.mark.parametrize("kind", ["flat0", "flat255", "noise", "natural", "rows"])
@pytest.mark.parametrize("ch", [1, 3])
def test_contents(kind, ch):
    for w, h in ((250, 65), (257, 200), (1100, 9)):   # 1100 bytes and more: the unrolled dword loop and its remainder
        frames = np.stack([_content(kind, w, h, ch, 7 + k) for k in range(2)])
        with api.Context(w, h, ch, 2) as ctx:
            got = _hist_view(ctx, frames, w * ch + 1, base_off=2)
            _same(got, frames, f"{kind} {w}x{h}x{ch}")
            if kind.startswith("flat"):   # every lane on one bin: the count is N
                v = 0 if kind == "flat0" else 255
                assert int(got[0, v]) == w * h * ch and int(got[0].sum()) == w * h * ch


def test_1080p_bgr_frame():
    frame = np.stack([synth.natural(1920, 1080, 31), synth.noise(1920, 1080, 32), synth.natural(1920, 1080, 33)], -1)[None]
    with api.Context(1920, 1080, 3, 1) as ctx:
        _same(ctx.histogram(frame), frame, "1920x1080x3")
        _same(_hist_view(ctx, frame, 5760 + 64, base_off=3), frame, "1920x1080x3 pitched, offset 3")


def test_batch_with_the_longest_chunk():
    """64 frames of 320 x 200: the batch is cut into 64-row chunks (the kernel's longest), the last of each frame 8 rows."""
    frames = np.stack([synth.natural(320, 200, 50 + k) if k % 3 else synth.flat(320, 200, k) for k in range(64)])
    with api.Context(320, 200, 1, 64) as ctx:
        _same(ctx.histogram(frames), frames, "64 x 320x200")


def test_second_call_into_the_same_table_gives_the_same_counts():
    import torch
    frames = np.stack([synth.natural(250, 65, 1), synth.noise(250, 65, 2)])
    d = torch.from_numpy(frames).cuda()
    hist = torch.zeros((2, 256), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with api.Context(250, 65, 1, 2) as ctx:
        for _ in range(2):
            ctx.histogram_device(d.data_ptr(), 250, 250 * 65, 2, hist.data_ptr())
        ctx.sync()
        _same(hist.cpu().numpy().view(np.uint32), frames, "called twice")


def test_callers_stream_is_honoured():
    """A torch op that writes the frames, queued before the call on the same stream with no sync in between, is seen."""
    import torch
    w, h, n = 640, 480, 8
    s = torch.cuda.Stream()
    d = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
    hist = torch.zeros((n, 256), dtype=torch.int32, device="cuda")
    big = torch.ones((4096, 4096), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with api.Context(w, h, 1, n) as ctx:
        ctx.set_stream(s.cuda_stream)
        with torch.cuda.stream(s):
            for _ in range(4):
                big = big @ big * 1e-4   # keeps the stream busy ahead of the write
            d.fill_(7)
            d[3].fill_(9)
        ctx.histogram_device(d.data_ptr(), w, w * h, n, hist.data_ptr())
        s.synchronize()
        got = hist.cpu().numpy()
        ctx.use_own_stream()
    for f in range(n):
        v = 9 if f == 3 else 7
        assert int(got[f, v]) == w * h and int(got[f].sum()) == w * h, (f, np.flatnonzero(got[f]).tolist())


def test_argument_errors():
    import torch
    d = torch.zeros((2, 8, 16), dtype=torch.uint8, device="cuda")
    hist = torch.zeros((2, 257), dtype=torch.int32, device="cuda")
    with api.Context(16, 8, 1, 2) as ctx:
        for args in ((0, 16, 128, 1, hist.data_ptr()), (d.data_ptr(), 16, 128, 1, 0), (d.data_ptr(), 16, 128, 1, hist.data_ptr() + 2),
                     (d.data_ptr(), 15, 128, 1, hist.data_ptr()), (d.data_ptr(), 16, 128, 0, hist.data_ptr()), (d.data_ptr(), 16, 128, 3, hist.data_ptr()),
                     (d.data_ptr(), 16, 127, 2, hist.data_ptr()), (d.data_ptr(), 1 << 29, 1 << 32, 1, hist.data_ptr())):
            with pytest.raises(api.HipCannyError, match="error -1"):
                ctx.histogram_device(*args)
        thr = torch.zeros((2, 2), dtype=torch.int32, device="cuda")
        for rule, param in ((2, 0.5), (-1, 0.5), (0, -0.1), (0, 1.5), (1, float("nan")), (1, float("inf"))):
            with pytest.raises(api.HipCannyError, match="error -1"):
                ctx.auto_thresholds_device(d.data_ptr(), 16, 128, 2, rule, param, thr.data_ptr())
        with pytest.raises(api.HipCannyError, match="error -1"):
            ctx.auto_thresholds_device(d.data_ptr(), 16, 128, 2, 0, 0.33, thr.data_ptr() + 1)
        with pytest.raises(api.HipCannyError, match="error -1"):
            ctx.auto_thresholds_device(d.data_ptr(), 15, 128, 2, 0, 0.33, thr.data_ptr())


# ---- automatic thresholds ----------------------------------------------------------------------------------------------
def _mixed(w, h, ch):
    two = np.where(np.arange(w)[None, :] < w // 3, 40, 180).astype(np.uint8) * np.ones((h, 1), np.uint8)
    half = np.where(np.arange(h)[:, None] < h // 2, 0, 255).astype(np.uint8) * np.ones((1, w), np.uint8)
    mono = [synth.flat(w, h, 0), synth.flat(w, h, 255), synth.flat(w, h, 93), two, half, synth.noise(w, h, 3), synth.natural(w, h, 4),
            synth.natural(w, h, 5) // 4, synth.steps(w, h, 200, "vertical")]
    if ch == 1:
        return np.stack(mono)
    return np.stack([np.stack([mono[k], mono[(k + 3) % len(mono)], mono[(k + 5) % len(mono)]], -1) for k in range(len(mono))])


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("w,h", [(64, 48), (250, 66), (1, 1), (2, 3)])
def test_auto_thresholds_equal_the_restatement(w, h, ch):
    import torch
    frames = _mixed(w, h, ch)
    n = frames.shape[0]
    d = torch.from_numpy(frames).cuda()
    thr = torch.full((n, 2), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with api.Context(w, h, ch, n, api.MODE_O) as ctx:
        for rule, params in ((api.AUTO_MEDIAN, (0.0, 0.33, 1.0)), (api.AUTO_OTSU, (0.0, 0.5, 1.0))):
            for p in params:
                ctx.auto_thresholds_device(d.data_ptr(), w * ch, w * ch * h, n, rule, p, thr.data_ptr())
                ctx.sync()
                got = [tuple(int(v) for v in row) for row in thr.cpu().numpy()]
                want = [R.thresholds(f, rule, p) for f in frames]
                assert got == want, (rule, p, got, want)


def test_canny_auto_equals_a_loop_of_single_frames():
    for ch in (1, 3):
        frames = _mixed(250, 66, ch)
        n = frames.shape[0]
        for rule, param in (("median", 0.33), ("otsu", 0.5)):
            with api.Context(250, 66, ch, n, api.MODE_O) as ctx:
                edges, thr = ctx.canny_auto(frames, rule, param)
                assert ctx.get_thresholds() == (50, 150)
            want_thr = [R.thresholds(f, rule, param) for f in frames]
            assert [tuple(int(v) for v in row) for row in thr] == want_thr
            with api.Context(250, 66, ch, 1, api.MODE_O) as one:
                for k in range(n):
                    want = one.canny(frames[k], want_thr[k][0], want_thr[k][1])[0]
                    assert np.array_equal(edges[k], want), (ch, rule, k, want_thr[k], int((edges[k] != want).sum()))
            assert any(e.any() for e in edges)
            if ch == 1:   # the three flat frames give empty maps
                assert not edges[:3].any()
