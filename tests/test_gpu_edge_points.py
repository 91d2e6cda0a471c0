"""hc_edge_points_device (k_edge_count, k_edge_scan, k_edge_emit) on the MI355X: counts and point lists equal, value for value and
in order, to the numpy restatement tests/edge_points_ref.py.  Every call runs on a map placed in a guarded arena
(tests/view_arena.py) that must come back unchanged, writes its counts between two guard words and its lists into a buffer
pre-filled with a canary (negative, so no coordinate) with guard space on both sides: everything but the first
min(count, capacity) pairs of each frame's slot must still hold the canary.

The shapes are the smallest at which the kernels' paths differ: rows shorter than a dword, ragged heads and tails at every base
offset, exactly one 64-dword trip, more than the four trips loaded together (1100 bytes), frames lower and higher than the
8-row chunk, one 1920 x 1080 pair and one 4100-wide map for the large coordinates.

Not asserted: that a call on a buffer no run writes leaves pipelined runs in flight -- every accessor that would show it
(hc_hysteresis_totals, hc_last_hysteresis_schedule, ...) completes the runs itself, so it cannot be observed without timing."""
import numpy as np
import pytest

import edge_points_ref as R
import view_arena as VA
from cudacam_amd import api, synth

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 5, 61, 64, 250, 257, 1100)
HEIGHTS = (1, 2, 65, 200)   # the chunk of these batches is 8 rows: 65 and 200 span several work items per frame
CANARY = -0x5A5A5A5B
GUARD = 64                  # int32 words of canary before and after the lists


def _content(kind, w, h, seed=0):
    rng = np.random.default_rng(1000 + seed)
    if kind == "zero":
        return np.zeros((h, w), np.uint8)
    if kind == "full":
        return np.full((h, w), 255, np.uint8)
    if kind == "corners":
        m = np.zeros((h, w), np.uint8)
        m[0, 0] = m[0, w - 1] = m[h - 1, 0] = 255
        m[h - 1, w - 1] = 7   # the last byte of the last row
        return m
    if kind == "mixed":   # 1 / 128 / 255 among zeros, as a THRESH map and worse
        return rng.choice(np.array([0, 0, 0, 1, 128, 255], np.uint8), size=(h, w))
    if kind == "noise":   # every second pixel, on average
        return np.where(rng.random((h, w)) < 0.5, rng.integers(1, 256, (h, w)), 0).astype(np.uint8)
    if kind == "sparse":
        return np.where(rng.random((h, w)) < 0.03, 255, 0).astype(np.uint8)
    raise ValueError(kind)


def _call(ctx, maps, capacity, pitch=None, frame_stride=None, base_off=0, fill="random", seed=0, null_points=False, what=""):
    """One call on `maps` (n, H, W) placed at pitch / frame stride / base offset in a guarded arena; everything is compared with
    the restatement.  Returns the counts."""
    import torch
    n, h, w = maps.shape
    pitch = w if pitch is None else pitch
    arena, off = VA.make_input(maps, pitch, frame_stride, base_off, fill, seed=seed)
    g = VA.input_geometry(maps, pitch, frame_stride, base_off)
    d = torch.from_numpy(arena).cuda()
    counts = torch.full((n + 2,), CANARY, dtype=torch.int32, device="cuda")
    pts = torch.full((2 * GUARD + 2 * n * capacity,), CANARY, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.edge_points_device(d.data_ptr() + off, pitch, g.frame_stride, n, counts.data_ptr() + 4,
                           None if null_points else pts.data_ptr() + 4 * GUARD, capacity)
    ctx.sync()
    assert np.array_equal(d.cpu().numpy(), arena), f"{what}: the input arena was written"
    c = counts.cpu().numpy()
    assert c[0] == CANARY and c[-1] == CANARY, f"{what}: a word beside d_counts was written"
    got_counts = c[1:-1].view(np.uint32)
    want_counts, want = R.edge_points(maps, capacity)
    assert got_counts.tolist() == want_counts.tolist(), f"{what}: counts {got_counts.tolist()} != {want_counts.tolist()}"
    p = pts.cpu().numpy()
    assert (p[:GUARD] == CANARY).all() and (p[len(p) - GUARD:] == CANARY).all(), f"{what}: the guard around d_points was written"
    slots = p[GUARD:len(p) - GUARD].reshape(n, capacity, 2)
    for f in range(n):
        k = len(want[f])
        assert k == min(int(want_counts[f]), capacity)
        if not np.array_equal(slots[f, :k], want[f]):
            bad = np.flatnonzero((slots[f, :k] != want[f]).any(axis=1))
            raise AssertionError(f"{what}: frame {f}: {len(bad)} of {k} points differ; first (index, hip, numpy): "
                                 f"{[(int(i), slots[f, i].tolist(), want[f][i].tolist()) for i in bad[:6]]}")
        assert (slots[f, k:] == CANARY).all(), f"{what}: frame {f}: the slot was written behind its {k} points"
    return got_counts


@pytest.mark.parametrize("w", WIDTHS)
def test_every_width_height_layout(w):
    for h in HEIGHTS:
        for n in (1, 3):
            maps = np.stack([_content(("noise", "sparse", "mixed")[(k + h) % 3], w, h, 10 * w + h + k) for k in range(n)])
            cap = w * h   # nothing is cut
            with api.Context(w, h, 1, 3, api.MODE_O if (w + h) % 2 else api.MODE_R) as ctx:   # either mode
                t = f"{w}x{h} n={n}"
                _call(ctx, maps, cap, what="tight " + t)
                # pitched rows, padding poisoned with 0xFF (a reader that strays counts it); a gap between the frames
                _call(ctx, maps, cap, VA.round_up(w, 4) + 8, (VA.round_up(w, 4) + 8) * h + 12, fill="ff", what="pitched " + t)
                for off in (1, 2, 3):   # the bytewise head and tail: base offsets, an odd pitch
                    _call(ctx, maps, cap, w + 3, (w + 3) * h + 5, base_off=off, fill="ff", seed=off, what=f"offset {off} " + t)
                # an ROI of a larger natural image: the neighbours are (non-zero) pixels of the parent
                _call(ctx, maps, cap, w + 37, base_off=11, fill="parent", what="ROI " + t)


@pytest.mark.parametrize("kind", ["zero", "full", "corners", "mixed", "noise"])
def test_contents(kind):
    for w, h in ((250, 65), (257, 200), (1100, 9), (3, 2)):
        maps = np.stack([_content(kind, w, h, 7 + k) for k in range(2)])
        with api.Context(w, h, 1, 2) as ctx:
            got = _call(ctx, maps, w * h, w + 1, base_off=2, fill="ff", what=f"{kind} {w}x{h}")
            if kind == "zero":
                assert got.tolist() == [0, 0]
            if kind == "full":
                assert got.tolist() == [w * h, w * h]
            if kind == "corners":
                assert got.tolist() == [len({(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)})] * 2


def test_canny_output_of_natural_frames():
    w, h, n = 250, 65, 3
    frames = np.stack([synth.natural(w, h, 40 + k) for k in range(n)])
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        maps = ctx.canny(frames, 50, 150)
        assert maps.any() and set(np.unique(maps).tolist()) <= {0, 255}
        _call(ctx, maps, int((maps != 0).sum(axis=(1, 2)).max()), what="canny maps")
        counts, lists = ctx.edge_points(maps)   # the two-pass convenience, host maps
        want_counts, want = R.edge_points(maps)
        assert counts.tolist() == want_counts.tolist()
        assert all(np.array_equal(a, b) and a.dtype == np.int32 for a, b in zip(lists, want))
        import torch
        counts, lists = ctx.edge_points(torch.from_numpy(maps).cuda(), capacity=10)   # torch maps, cut lists
        assert counts.tolist() == want_counts.tolist()
        assert all(np.array_equal(a, b[:10]) for a, b in zip(lists, want))


def test_capacities():
    w, h = 250, 65
    maps = np.stack([_content("sparse", w, h, 1), _content("noise", w, h, 2)])
    cs = [R.count(m) for m in maps]
    assert 5 < cs[0] < cs[1]
    with api.Context(w, h, 1, 2) as ctx:
        _call(ctx, maps, 0, null_points=True, what="capacity 0, NULL")
        _call(ctx, maps, 0, what="capacity 0, a pointer")
        for cap in (1, cs[0] - 1, cs[0], cs[0] + 5, cs[1] - 1, cs[1], cs[1] + 5):   # cs[0] + 5: one frame under, one over
            _call(ctx, maps, cap, w + 3, base_off=1, fill="ff", what=f"capacity {cap}")
        _call(ctx, maps[:1], cs[0] - 1, what="one frame, count - 1")


def test_cut_inside_a_row_and_inside_a_trip():
    w, h = 1100, 9
    maps = np.full((2, h, w), 255, np.uint8)
    with api.Context(w, h, 1, 2) as ctx:
        for cap in (300, w + 300):
            for off in (0, 3):   # with and without head bytes: the cut falls on other lanes
                _call(ctx, maps, cap, w + 4, base_off=off, fill="ff", what=f"all 255, capacity {cap}, offset {off}")


def test_larger_coordinates():
    maps = np.full((2, 1080, 1920), 255, np.uint8)
    with api.Context(1920, 1080, 1, 2) as ctx:
        got = _call(ctx, maps, 1920 * 1080, what="1920x1080 all 255")
        assert got.tolist() == [2073600, 2073600]
    wide = _content("noise", 4100, 9, 3)[None]
    with api.Context(4100, 9, 1, 1) as ctx:
        _call(ctx, wide, 4100 * 9, 4100 + 5, base_off=1, fill="ff", what="4100x9")


def test_other_chunk_lengths_and_many_chunks():
    """1024 frames of 16 x 65 are cut into 9-row chunks (the rule leaves its 8-row floor above 65536 rows per call), the last of
    each frame 2 rows; one frame of 16 x 1100 into 138 chunks of 8 rows: more than the 64 the scan takes per trip."""
    maps = np.stack([_content("sparse" if k % 3 else "noise", 16, 65, 50 + k % 7) for k in range(1024)])
    with api.Context(16, 65, 1, 1024) as ctx:
        _call(ctx, maps, 16 * 65, what="1024 x 16x65")
    tall = _content("noise", 16, 1100, 9)[None]
    with api.Context(16, 1100, 1, 1) as ctx:
        _call(ctx, tall, 16 * 1100, 19, base_off=1, what="16x1100")


def test_not_a_run():
    w, h, n = 250, 65, 2
    frames = np.stack([synth.natural(w, h, 60 + k) for k in range(n)])
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        maps = ctx.canny(frames, 50, 150)
        before = (ctx.hysteresis_schedule(), ctx.last_run_info(), ctx.pipeline_slots_in_use(), ctx.hysteresis_totals(), ctx.hysteresis_info())
        assert before[0]["launches"] > 0
        _call(ctx, maps, w * h, what="after a run")
        _call(ctx, maps, 0, null_points=True, what="after a run, counts only")
        after = (ctx.hysteresis_schedule(), ctx.last_run_info(), ctx.pipeline_slots_in_use(), ctx.hysteresis_totals(), ctx.hysteresis_info())
        assert before == after


def test_after_pipelined_runs_without_a_sync():
    """Two pipelined runs into two buffers, then the lists of the FIRST buffer with no synchronisation in between: the entry
    completes the run that writes the map it reads."""
    import torch
    w, h, n = 640, 480, 8
    a = np.stack([synth.natural(w, h, 70 + k) for k in range(n)])
    b = np.stack([synth.natural(w, h, 90 + k) for k in range(n)])
    d_in = [torch.from_numpy(v).cuda() for v in (a, b)]
    outs = [torch.zeros((n, h, w), dtype=torch.uint8, device="cuda") for _ in range(2)]
    other = torch.from_numpy(_content("sparse", w, h, 5)[None].repeat(n, 0)).cuda()
    cap = w * h // 4
    counts = torch.full((3, n), CANARY, dtype=torch.int32, device="cuda")
    pts = torch.full((n, cap, 2), CANARY, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with api.Context(w, h, 1, n, api.MODE_R) as ctx:
        ctx.set_option(api.OPT_PIPELINE, 1)
        for r in range(2):
            ctx.run_device(d_in[r].data_ptr(), w, w * h, outs[r].data_ptr(), w, w * h, n)
        ctx.edge_points_device(other.data_ptr(), w, w * h, n, counts[2].data_ptr(), None, 0)   # a buffer no run writes
        ctx.edge_points_device(outs[0].data_ptr(), w, w * h, n, counts[0].data_ptr(), pts.data_ptr(), cap)
        ctx.sync()
        maps = outs[0].cpu().numpy()
        assert maps.any()
        want_counts, want = R.edge_points(maps, cap)
        assert counts[0].cpu().numpy().view(np.uint32).tolist() == want_counts.tolist()
        assert int(want_counts.max()) < cap
        p = pts.cpu().numpy()
        for f in range(n):
            assert np.array_equal(p[f, :len(want[f])], want[f]), f
            assert (p[f, len(want[f]):] == CANARY).all()
        assert counts[2].cpu().numpy().view(np.uint32).tolist() == [R.count(m) for m in other.cpu().numpy()]
        # the second buffer, now complete as well
        ctx.edge_points_device(outs[1].data_ptr(), w, w * h, n, counts[1].data_ptr(), None, 0)
        ctx.sync()
        assert counts[1].cpu().numpy().view(np.uint32).tolist() == [R.count(m) for m in outs[1].cpu().numpy()]


@pytest.mark.parametrize("aperture", [3, 7])
def test_canny_points(aperture):
    w, h, n = 250, 65, 3
    frames = np.stack([synth.natural(w, h, 80 + k) for k in range(n)])
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        want_maps = ctx.canny(frames, 50, 150, aperture)
        assert want_maps.any()
        for cap in (None, 20):
            maps, counts, lists = ctx.canny_points(frames, 50, 150, aperture, capacity=cap)
            assert np.array_equal(maps, want_maps)
            want_counts, want = R.edge_points(maps, cap)
            assert counts.tolist() == want_counts.tolist()
            assert len(lists) == n and all(np.array_equal(x, y) and x.dtype == np.int32 and x.shape == y.shape for x, y in zip(lists, want))


def test_argument_errors():
    import torch
    w, h = 16, 8
    d = torch.full((2, h, w), 255, dtype=torch.uint8, device="cuda")
    counts = torch.full((4,), CANARY, dtype=torch.int32, device="cuda")
    pts = torch.full((2 * 8 * 2 + 4,), CANARY, dtype=torch.int32, device="cuda")
    m, c, p = d.data_ptr(), counts.data_ptr(), pts.data_ptr()
    assert p % 8 == 0 and c % 4 == 0
    torch.cuda.synchronize()
    big = (1 << 64) // 8
    with api.Context(w, h, 1, 2) as ctx:
        bad = [
            (0, w, w * h, 1, c, p, 8),                   # d_map null
            (m, w, w * h, 1, 0, p, 8),                   # d_counts null
            (m, w, w * h, 1, c, 0, 8),                   # d_points null with capacity > 0
            (m, w, w * h, 1, c + 2, p, 8),               # d_counts misaligned
            (m, w, w * h, 1, c, p + 4, 8),               # d_points misaligned
            (m, w - 1, w * h, 1, c, p, 8),               # pitch < width
            (m, w, w * h, 0, c, p, 8),                   # nframes outside 1..max_batch
            (m, w, w * h, -1, c, p, 8),
            (m, w, w * h, 3, c, p, 8),
            (m, w, w * h - 1, 2, c, p, 8),               # frame stride smaller than a frame
            (m, 1 << 29, 1 << 32, 1, c, p, 8),           # height * pitch >= 2^32
            (m, w, w * h, 2, c, p, big // 2),            # capacity * 8 * nframes overflows size_t
            (m, w, w * h, 1, c, p, big),
        ]
        for args in bad:
            with pytest.raises(api.HipCannyError, match="error -1"):
                ctx.edge_points_device(*args)
        assert api.load_library().hc_edge_points_device(None, m, w, w * h, 1, c, p, 8) == -1   # ctx null
        ctx.sync()
        torch.cuda.synchronize()
        assert (counts.cpu().numpy() == CANARY).all() and (pts.cpu().numpy() == CANARY).all()
        ctx.edge_points_device(m, w, w * h, 2, c, p, 8)   # the same buffers are fine for a good call
        ctx.sync()
        assert counts.cpu().numpy()[:2].tolist() == [w * h, w * h]
    # with HC_OPT_PER_CHANNEL the bound is that of the run's output frames: 3 maps per input frame
    with api.Context(w, h, 3, 1) as ctx:
        three = torch.full((3, h, w), 255, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(api.HipCannyError, match="error -1"):
            ctx.edge_points_device(three.data_ptr(), w, w * h, 3, c, 0, 0)
        ctx.set_option(api.OPT_PER_CHANNEL, 1)
        ctx.edge_points_device(three.data_ptr(), w, w * h, 3, c, 0, 0)
        ctx.sync()
        assert counts.cpu().numpy()[:3].tolist() == [w * h] * 3
        with pytest.raises(api.HipCannyError, match="error -1"):
            ctx.edge_points_device(three.data_ptr(), w, w * h, 4, c, 0, 0)
