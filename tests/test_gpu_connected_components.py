"""hc_connected_components_device (ccl.hip) on the MI355X: labels, counts, statistics words and centroids (as float64 bit
patterns) equal, value for value, to the restatement tests/ccl_ref.py (numpy and a flood fill).

Every call reads its maps from a guarded arena (tests/view_arena.py) that must come back unchanged, writes its labels into a
canary-filled pitched arena in which only [row, row + 4 W) of each row may change, and its counts, statistics and centroids
between canary guards, the slot tails behind min(N, capacity) rows untouched.

The shapes are the smallest at which the paths differ: a tile is 64 x 32 pixels, so 65 x 64 is 2 x 2 tiles, 130 x 67 is 3 x 3 with
ragged last tiles and 200 x 150 is 4 x 5; rows of 8 make a chunk, so every size above 8 rows has several chunks per frame."""
import numpy as np
import pytest

import ccl_ref as R
import view_arena as VA
from cudacam_amd import api, synth

pytestmark = pytest.mark.gpu

SIZES = ((1, 1), (1, 70), (70, 1), (9, 7), (65, 64), (130, 67), (200, 150))   # W x H
CANARY = -0x5A5A5A5B
CANARY64 = -0x5A5A5A5A5A5A5A5B
GUARD = 64

_REF = {}


def _ref(maps, conn):
    """The restatement of a batch, computed once per (content, connectivity) and shared: every row, never modified."""
    key = (maps.shape, maps.tobytes(), conn)
    if key not in _REF:
        _REF[key] = R.connected_components(maps, conn)
    return _REF[key]


def _random(w, h, density, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.random((h, w)) < density, 255, 0).astype(np.uint8)


def _spiral(w, h):
    """A one-pixel path from the corner inwards, arms one pixel apart: one component with the deepest chains of links."""
    m = np.zeros((h, w), np.uint8)
    x = y = 0
    dx, dy = 1, 0
    m[0, 0] = 255
    free = lambda xx, yy: 0 <= xx < w and 0 <= yy < h and not m[yy, xx]
    beyond = lambda xx, yy: not (0 <= xx < w and 0 <= yy < h) or not m[yy, xx]
    turns = 0
    while turns < 2:
        if free(x + dx, y + dy) and beyond(x + 2 * dx, y + 2 * dy):
            x, y = x + dx, y + dy
            m[y, x] = 255
            turns = 0
        else:
            dx, dy = -dy, dx
            turns += 1
    return m


def _comb(w, h):
    """Every second row full, joined at alternating ends: one serpentine across all tiles, merged at hundreds of border pixels."""
    m = np.zeros((h, w), np.uint8)
    m[::2] = 255
    m[1::4, w - 1] = 255
    m[3::4, 0] = 255
    return m


def _content(kind, w, h, seed=0):
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "empty":
        return np.zeros((h, w), np.uint8)
    if kind == "full":
        return np.full((h, w), 255, np.uint8)
    if kind == "corners":
        m = np.zeros((h, w), np.uint8)
        m[0, 0] = m[0, w - 1] = m[h - 1, 0] = 255
        m[h - 1, w - 1] = 7
        return m
    if kind == "diagonal":
        return np.where(xx == yy, 255, 0).astype(np.uint8)
    if kind == "antidiagonal":
        return np.where(xx + yy == min(w, h) - 1, 255, 0).astype(np.uint8)
    if kind == "checkerboard":
        return np.where((xx + yy) % 2 == 0, 255, 0).astype(np.uint8)
    if kind == "grid":
        m = np.zeros((h, w), np.uint8)
        m[::2, ::2] = 255
        return m
    if kind == "spiral":
        return _spiral(w, h)
    if kind == "comb":
        return _comb(w, h)
    if kind == "mixed":   # 1 / 128 / 255 among zeros, as a THRESH map and worse
        return np.random.default_rng(seed).choice(np.array([0, 0, 1, 128, 255], np.uint8), size=(h, w))
    if kind.startswith("random"):
        return _random(w, h, float(kind[6:]), 1000 + seed)
    raise ValueError(kind)


def _call(ctx, maps, conn, capacity, pitch=None, frame_stride=None, base_off=0, label_pad=0, label_gap=0, label_off=0, fill="ff", null_rows=False, what="", want=None):
    """One call on `maps` (n, H, W) in a guarded arena; everything is compared with the restatement -- or with `want`, the same four
    values from a closed form (ccl_ref.checkerboard4, ccl_ref.columns) where a flood fill would take too long.  Returns (labels, counts)."""
    import torch
    n, h, w = maps.shape
    pitch = w if pitch is None else pitch
    arena, off = VA.make_input(maps, pitch, frame_stride, base_off, fill, seed=w + h)
    g = VA.input_geometry(maps, pitch, frame_stride, base_off)
    lpitch = 4 * w + label_pad
    larena, lg = VA.make_output(n, h, 4 * w, lpitch, lpitch * h + label_gap, label_off, seed=w)
    d = torch.from_numpy(arena).cuda()
    dl = torch.from_numpy(larena).cuda()
    counts = torch.full((n + 2,), CANARY, dtype=torch.int32, device="cuda")
    stats = torch.full((2 * GUARD + 5 * n * capacity,), CANARY, dtype=torch.int32, device="cuda")
    cents = torch.full((2 * GUARD + 2 * n * capacity,), CANARY64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.connected_components_device(d.data_ptr() + off, pitch, g.frame_stride, n, conn, dl.data_ptr() + lg.offset, lpitch, lg.frame_stride, counts.data_ptr() + 4,
                                    None if null_rows else stats.data_ptr() + 4 * GUARD, None if null_rows else cents.data_ptr() + 8 * GUARD, capacity)
    ctx.sync()
    want_labels, want_counts, want_stats, want_cents = _ref(maps, conn) if want is None else want
    assert np.array_equal(d.cpu().numpy(), arena), f"{what}: the map arena was written"
    c = counts.cpu().numpy()
    assert c[0] == CANARY and c[-1] == CANARY, f"{what}: a word beside d_counts was written"
    got_counts = c[1:-1].view(np.uint32)
    assert got_counts.tolist() == want_counts.tolist(), f"{what}: counts {got_counts.tolist()} != {want_counts.tolist()}"
    VA.check_output(dl.cpu().numpy(), larena, lg, want_labels, what=f"{what}: labels")
    s, q = stats.cpu().numpy(), cents.cpu().numpy()
    assert (s[:GUARD] == CANARY).all() and (s[len(s) - GUARD:] == CANARY).all(), f"{what}: the guard around d_stats was written"
    assert (q[:GUARD] == CANARY64).all() and (q[len(q) - GUARD:] == CANARY64).all(), f"{what}: the guard around d_centroids was written"
    s, q = s[GUARD:len(s) - GUARD].reshape(n, capacity, 5), q[GUARD:len(q) - GUARD].reshape(n, capacity, 2)
    for f in range(n):
        k = min(int(want_counts[f]), capacity)
        if not np.array_equal(s[f, :k], want_stats[f][:k]):
            bad = np.flatnonzero((s[f, :k] != want_stats[f][:k]).any(axis=1))
            raise AssertionError(f"{what}: frame {f}: {len(bad)} of {k} statistics rows differ; first (row, hip, numpy): "
                                 f"{[(int(i), s[f, i].tolist(), want_stats[f][i].tolist()) for i in bad[:6]]}")
        wc = want_cents[f][:k].view(np.int64)
        if not np.array_equal(q[f, :k], wc):
            bad = np.flatnonzero((q[f, :k] != wc).any(axis=1))
            raise AssertionError(f"{what}: frame {f}: {len(bad)} of {k} centroids differ in their bits; first (row, hip, numpy): "
                                 f"{[(int(i), q[f, i].view(np.float64).tolist(), want_cents[f][i].tolist()) for i in bad[:6]]}")
        assert (s[f, k:] == CANARY).all() and (q[f, k:] == CANARY64).all(), f"{what}: frame {f}: a slot was written behind its {k} rows"
    return want_labels, got_counts


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_size_layout_and_connectivity(size):
    w, h = size
    for n in (1, 3):
        maps = np.stack([_content(("random0.3", "random0.5", "mixed")[k % 3], w, h, 10 * w + h + k) for k in range(n)])
        cap = w * h + 1   # nothing is cut
        with api.Context(w, h, 1, 3, api.MODE_O if (w + h) % 2 else api.MODE_R) as ctx:   # either mode
            for conn in (4, 8):
                t = f"{w}x{h} n={n} c={conn}"
                _call(ctx, maps, conn, cap, what="tight " + t)
                # ragged dword heads and tails: base offsets 0..3 at an odd pitch, the padding poisoned with 0xFF (a reader that
                # strays labels it); the label rows padded, a gap between the frames on both sides, the labels an ROI of a plane
                for off in (0, 1, 2, 3):
                    _call(ctx, maps, conn, cap, w + 3, (w + 3) * h + 5, base_off=off, label_pad=4 * (off + 1), label_gap=8 * off, label_off=4 * off, what=f"offset {off} " + t)
            _call(ctx, maps, 8, cap, w + 37, base_off=11, fill="parent", label_pad=44, label_off=20, what=f"ROI {w}x{h} n={n}")


@pytest.mark.parametrize("kind", ["empty", "full", "corners", "diagonal", "antidiagonal", "checkerboard", "grid", "spiral", "comb", "mixed",
                                  "random0.03", "random0.3", "random0.5", "random0.6"])
def test_contents(kind):
    for w, h in ((200, 150), (130, 67), (9, 7)):
        maps = np.stack([_content(kind, w, h, 7 + k) for k in range(2)])
        with api.Context(w, h, 1, 2) as ctx:
            for conn in (4, 8):
                _, got = _call(ctx, maps, conn, w * h + 1, w + 1, base_off=2, label_pad=12, what=f"{kind} {w}x{h} c={conn}")
                n = int(got[0])
                if kind == "empty":
                    assert n == 1
                if kind in ("full", "spiral", "comb"):
                    assert n == 2
                if kind == "diagonal":
                    assert n == (2 if conn == 8 else min(w, h) + 1)
                if kind == "checkerboard":
                    assert n == (2 if conn == 8 else (w * h + 1) // 2 + 1)
                if kind == "grid":
                    assert n == ((w + 1) // 2) * ((h + 1) // 2) + 1 and ((w, h) != (200, 150) or n == 7501)


def test_blobs_that_touch_through_the_corner_of_four_tiles():
    w, h = 200, 150
    m = np.zeros((h, w), np.uint8)
    m[28:32, 60:64] = 255    # ends at the corner (64, 32) of four tiles ...
    m[32:36, 64:68] = 255    # ... and begins there: the two share that corner only
    m[60:64, 128:132] = 9    # the other diagonal, at the corner (128, 64)
    m[64:68, 124:128] = 9
    m[96, 191] = m[95, 192] = 1   # single pixels across the corner (192, 96)
    with api.Context(w, h, 1, 1) as ctx:
        assert _call(ctx, m[None], 8, 16, what="corner blobs, 8")[1].tolist() == [4]
        assert _call(ctx, m[None], 4, 16, what="corner blobs, 4")[1].tolist() == [7]


def test_frames_of_a_batch_are_independent():
    w, h = 130, 67
    kinds = ("comb", "empty", "random0.5", "full", "grid", "spiral", "random0.6")
    maps = np.stack([_content(k, w, h, 3) for k in kinds])
    with api.Context(w, h, 1, len(kinds)) as ctx:
        for conn in (4, 8):
            _call(ctx, maps, conn, w * h + 1, w + 5, (w + 5) * h + 77, base_off=3, label_pad=20, label_gap=4 * 333, what=f"seven contents c={conn}")
            for f in (0, 2, 6):   # each frame alone gives the same rows (the restatement is per frame; the device must be too)
                _call(ctx, maps[f:f + 1], conn, w * h + 1, what=f"frame {f} alone c={conn}")


def test_capacities():
    w, h = 130, 67
    maps = np.stack([_content("random0.03", w, h, 1), _content("random0.3", w, h, 2)])
    ns = [int(v) for v in _ref(maps, 8)[1]]
    assert 5 < ns[0] < ns[1]
    with api.Context(w, h, 1, 2) as ctx:
        _call(ctx, maps, 8, 0, null_rows=True, what="capacity 0, NULL")
        _call(ctx, maps, 8, 0, what="capacity 0, pointers")
        for cap in (1, ns[0] - 1, ns[0], ns[0] + 5, ns[1] - 1, ns[1], ns[1] + 5):   # 1: the background rows only
            _call(ctx, maps, 8, cap, w + 3, base_off=1, label_pad=8, what=f"capacity {cap}")
        full = np.full((1, h, w), 255, np.uint8)   # the background row is the all-zero row
        for cap in (1, 2, 3):
            _call(ctx, full, 4, cap, what=f"full frame, capacity {cap}")


def test_several_passes_under_a_small_scratch_bound():
    """67 rows are 9 chunks of 8: 36 bytes of table per frame.  A bound of 80 bytes cuts five frames into passes of 2, 2 and 1."""
    w, h = 130, 67
    maps = np.stack([_content(("random0.5", "comb", "grid", "random0.3", "spiral")[k], w, h, k) for k in range(5)])
    with api.Context(w, h, 1, 5) as ctx:
        ctx.set_option(api.OPT_TEST_HOUGH_SCRATCH, 80)
        _call(ctx, maps, 8, 3000, w + 2, (w + 2) * h + 9, base_off=1, label_pad=4, label_gap=40, what="passes of two frames")
        ctx.set_option(api.OPT_TEST_HOUGH_SCRATCH, 36)
        _call(ctx, maps, 4, 3000, what="a pass per frame")
        ctx.set_option(api.OPT_TEST_HOUGH_SCRATCH, 35)
        with pytest.raises(api.HipCannyError, match="scratch bound"):
            _call(ctx, maps, 4, 3000, what="a bound below one frame")
        ctx.set_option(api.OPT_TEST_HOUGH_SCRATCH, 0)
        _call(ctx, maps, 4, 3000, what="the default bound again")


def test_canny_components_and_a_thresh_map():
    w, h, n = 200, 150, 2
    frames = np.stack([synth.natural(w, h, 40 + k) for k in range(n)])
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        want_maps = ctx.canny(frames, 50, 150)
        assert want_maps.any()
        for conn in (4, 8):
            want = _ref(want_maps, conn)
            for cap in (None, 5):
                maps, labels, counts, stats, cents = ctx.canny_components(frames, 50, 150, conn, max_components=cap)
                assert np.array_equal(maps, want_maps) and np.array_equal(labels, want[0]) and labels.dtype == np.int32
                assert counts.tolist() == want[1].tolist() and int(counts.min()) > 5
                for f in range(n):
                    k = int(counts[f]) if cap is None else cap
                    assert np.array_equal(stats[f], want[2][f][:k]) and np.array_equal(cents[f].view(np.int64), want[3][f][:k].view(np.int64))
            _call(ctx, want_maps, conn, int(want[1].max()), w + 1, base_off=1, what=f"canny maps c={conn}")
        labels, counts, stats, cents = ctx.connected_components(want_maps[0])   # one host map, the defaults
        assert np.array_equal(labels[0], _ref(want_maps, 8)[0][0]) and len(stats[0]) == int(counts[0])
    with api.Context(w, h, 1, n, api.MODE_R) as ctx:   # the 0 / 128 / 255 of an HC_STAGE_THRESH map: both values are foreground
        ctx.upload(frames)
        ctx.run(api.CannyStage.THRESH, n)
        thr = ctx.download(n)
        assert {128, 255} <= set(np.unique(thr).tolist())
        _call(ctx, thr, 8, w * h, what="THRESH map")


def test_not_a_run():
    w, h, n = 200, 150, 2
    frames = np.stack([synth.natural(w, h, 60 + k) for k in range(n)])
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        maps = ctx.canny(frames, 50, 150)
        before = (ctx.hysteresis_schedule(), ctx.last_run_info(), ctx.pipeline_slots_in_use(), ctx.hysteresis_totals(), ctx.hysteresis_info())
        assert before[0]["launches"] > 0
        _call(ctx, maps, 8, w * h, what="after a run")
        _call(ctx, maps, 4, 0, null_rows=True, what="after a run, labels only")
        after = (ctx.hysteresis_schedule(), ctx.last_run_info(), ctx.pipeline_slots_in_use(), ctx.hysteresis_totals(), ctx.hysteresis_info())
        assert before == after


def test_behind_pipelined_runs_without_a_sync_and_scratch_growth_while_queued():
    """Two pipelined runs into two buffers, then the components of the FIRST buffer with no synchronisation in between: the entry
    completes the run that writes the map it reads.  The first call takes one frame, the second, queued behind it, all of them: the
    table grows while the first call may still be running."""
    import torch
    w, h, n = 320, 240, 6
    a = np.stack([synth.natural(w, h, 70 + k) for k in range(n)])
    b = np.stack([synth.natural(w, h, 90 + k) for k in range(n)])
    d_in = [torch.from_numpy(v).cuda() for v in (a, b)]
    outs = [torch.zeros((n, h, w), dtype=torch.uint8, device="cuda") for _ in range(2)]
    cap = 4096
    labels = [torch.full((k, h, w), CANARY, dtype=torch.int32, device="cuda") for k in (1, n, n)]
    counts = torch.full((3, n), CANARY, dtype=torch.int32, device="cuda")
    stats = torch.full((n, cap, 5), CANARY, dtype=torch.int32, device="cuda")
    cents = torch.full((n, cap, 2), CANARY64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with api.Context(w, h, 1, n, api.MODE_R) as ctx:
        ctx.set_option(api.OPT_PIPELINE, 1)
        for r in range(2):
            ctx.run_device(d_in[r].data_ptr(), w, w * h, outs[r].data_ptr(), w, w * h, n)
        ctx.connected_components_device(outs[0].data_ptr(), w, w * h, 1, 8, labels[0].data_ptr(), 4 * w, 4 * w * h, counts[0].data_ptr())
        ctx.connected_components_device(outs[0].data_ptr(), w, w * h, n, 8, labels[1].data_ptr(), 4 * w, 4 * w * h, counts[1].data_ptr(), stats.data_ptr(), cents.data_ptr(), cap)
        ctx.connected_components_device(outs[1].data_ptr(), w, w * h, n, 4, labels[2].data_ptr(), 4 * w, 4 * w * h, counts[2].data_ptr())
        ctx.sync()
        maps = [o.cpu().numpy() for o in outs]
        assert maps[0].any() and maps[1].any()
        want = _ref(maps[0], 8)
        assert int(want[1].max()) <= cap
        assert np.array_equal(labels[0].cpu().numpy()[0], want[0][0]) and counts[0].cpu().numpy().view(np.uint32)[0] == want[1][0]
        assert np.array_equal(labels[1].cpu().numpy(), want[0]) and counts[1].cpu().numpy().view(np.uint32).tolist() == want[1].tolist()
        s, q = stats.cpu().numpy(), cents.cpu().numpy()
        for f in range(n):
            k = int(want[1][f])
            assert np.array_equal(s[f, :k], want[2][f]) and np.array_equal(q[f, :k], want[3][f].view(np.int64)), f
            assert (s[f, k:] == CANARY).all() and (q[f, k:] == CANARY64).all(), f
        want4 = _ref(maps[1], 4)
        assert np.array_equal(labels[2].cpu().numpy(), want4[0]) and counts[2].cpu().numpy().view(np.uint32).tolist() == want4[1].tolist()


def test_argument_errors():
    import torch
    w, h = 16, 8
    d = torch.full((2, h, w), 255, dtype=torch.uint8, device="cuda")
    lab = torch.full((2 * h * w + 8,), CANARY, dtype=torch.int32, device="cuda")
    counts = torch.full((4,), CANARY, dtype=torch.int32, device="cuda")
    stats = torch.full((2 * 8 * 5 + 4,), CANARY, dtype=torch.int32, device="cuda")
    cents = torch.full((2 * 8 * 2 + 4,), CANARY64, dtype=torch.int64, device="cuda")
    both = torch.full((5 * h * w + 64,), 255, dtype=torch.uint8, device="cuda")   # a map with its labels right behind it
    m, l, c, s, q, u = d.data_ptr(), lab.data_ptr(), counts.data_ptr(), stats.data_ptr(), cents.data_ptr(), both.data_ptr()
    assert l % 4 == 0 and c % 4 == 0 and s % 4 == 0 and q % 8 == 0 and u % 4 == 0
    torch.cuda.synchronize()
    fs, lp, lfs = w * h, 4 * w, 4 * w * h
    big = 1 << 64
    with api.Context(w, h, 1, 2) as ctx:
        good = (m, w, fs, 1, 8, l, lp, lfs, c, s, q, 8)
        bad = {
            "d_map null": (0,) + good[1:],
            "d_labels null": good[:5] + (0,) + good[6:],
            "d_counts null": good[:8] + (0,) + good[9:],
            "d_stats null with capacity > 0": good[:9] + (0, q, 8),
            "d_centroids null with capacity > 0": good[:9] + (s, 0, 8),
            "connectivity 6": good[:4] + (6,) + good[5:],
            "connectivity 0": good[:4] + (0,) + good[5:],
            "d_counts misaligned": good[:8] + (c + 2,) + good[9:],
            "d_stats misaligned": good[:9] + (s + 2, q, 8),
            "d_centroids misaligned": good[:9] + (s, q + 4, 8),
            "d_labels misaligned": good[:5] + (l + 2,) + good[6:],
            "label_pitch no multiple of 4": good[:6] + (lp + 2,) + good[7:],
            "label_frame_stride no multiple of 4": (m, w, fs, 2, 8, l, lp, lfs + 2, c, s, q, 8),
            "pitch < W": (m, w - 1) + good[2:],
            "label_pitch < 4 W": good[:6] + (lp - 4,) + good[7:],
            "nframes 0": good[:3] + (0,) + good[4:],
            "nframes -1": good[:3] + (-1,) + good[4:],
            "nframes 3 of 2": good[:3] + (3,) + good[4:],
            "map frame stride below a frame": (m, w, fs - 1, 2, 8, l, lp, lfs, c, s, q, 8),
            "label frame stride below a frame": (m, w, fs, 2, 8, l, lp, lfs - 4, c, s, q, 8),
            "H * pitch >= 2^32": (m, 1 << 29, 1 << 32) + good[3:],
            "H * label_pitch >= 2^32": good[:6] + (1 << 29, 1 << 32) + good[8:],
            "a map that wraps the address space": (big - 64,) + good[1:],
            "labels that wrap the address space": good[:5] + (big - 64,) + good[6:],
            "labels inside the map": (u, w, fs, 1, 8, u + fs - 4, lp, lfs, c, s, q, 8),
            "the map inside the labels": (u + 4, w, fs, 1, 8, u, lp, lfs, c, s, q, 8),
            "capacity * 20 * nframes overflows": (m, w, fs, 2, 8, l, lp, lfs, c, s, q, big // 20 // 2 + 1),
            "capacity * 16 * nframes overflows": (m, w, fs, 2, 8, l, lp, lfs, c, s, q, big // 16 // 2 + 1),
        }
        for name, args in bad.items():
            with pytest.raises(api.HipCannyError, match="error -1"):
                ctx.connected_components_device(*args)
            assert "hc_connected_components_device: " in api.last_error(), name
        assert api.load_library().hc_connected_components_device(None, *good) == -1   # ctx null
        ctx.sync()
        torch.cuda.synchronize()
        for t in (lab, counts, stats):
            assert (t.cpu().numpy() == CANARY).all()
        assert (cents.cpu().numpy() == CANARY64).all()
        # views that merely touch are fine: the labels begin where the map ends
        ctx.connected_components_device(u, w, fs, 1, 8, u + fs, lp, lfs, c, s, q, 8)
        ctx.connected_components_device(m, w, fs, 2, 4, l, lp, lfs, c + 4, s, q, 8)   # the same buffers are fine for a good call
        ctx.sync()
        assert counts.cpu().numpy()[:3].tolist() == [2, 2, 2]
        assert (both.cpu().numpy()[:fs] == 255).all() and (both.cpu().numpy()[fs:fs + lfs].view(np.int32) == 1).all()
        assert (lab.cpu().numpy()[:2 * h * w] == 1).all() and (lab.cpu().numpy()[2 * h * w:] == CANARY).all()
        assert stats.cpu().numpy()[:10].tolist() == [0, 0, 0, 0, 0, 0, 0, w, h, w * h]
    # with HC_OPT_PER_CHANNEL the bound is that of the run's output frames: 3 maps per input frame
    with api.Context(w, h, 3, 1) as ctx:
        three = torch.full((3, h, w), 255, dtype=torch.uint8, device="cuda")
        lab3 = torch.empty((3, h, w), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(api.HipCannyError, match="error -1"):
            ctx.connected_components_device(three.data_ptr(), w, fs, 3, 8, lab3.data_ptr(), lp, lfs, c)
        ctx.set_option(api.OPT_PER_CHANNEL, 1)
        ctx.connected_components_device(three.data_ptr(), w, fs, 3, 8, lab3.data_ptr(), lp, lfs, c)
        ctx.sync()
        assert counts.cpu().numpy()[:3].tolist() == [2, 2, 2] and (lab3.cpu().numpy() == 1).all()
        with pytest.raises(api.HipCannyError, match="error -1"):
            ctx.connected_components_device(three.data_ptr(), w, fs, 4, 8, lab3.data_ptr(), lp, lfs, c)


# ---- the tall and large paths: the thresholds follow from the constants of ccl.hip and canny_params.h.  k_ccl_scan takes a frame's
# chunks 64 at a time (a carry from 513 rows of 8 up), hist_chunk_rows leaves 8 rows per chunk once H x nframes passes 65,536,
# k_ccl_rows and k_ccl_finish stride over the rows from CCL_ROW_GROUPS x CCL_THREADS = 262,144 up, and a sum of coordinates passes
# 2^32 once W * H * (H - 1) / 2 does.  Each shape is narrow or short in the other direction, so that it stays small.
ROW_THREADS = 1024 * 256


@pytest.mark.parametrize("kind", ["random0.3", "comb", "spiral"])
def test_the_scan_carries_across_64_chunks(kind):
    """65 x 520, two frames: 65 chunks of 8 rows, one carry in k_ccl_scan, and k_ccl_roots numbers across it.  9 x 1030: 129
    chunks, two carries.  A carry that is dropped, or added twice, shifts every number behind chunk 64."""
    for w, h, n in ((65, 520, 2), (9, 1030, 1)):
        assert (h + 7) // 8 > 64 * (2 if h > 1024 else 1) and h * n <= 65536
        maps = np.stack([_content(kind, w, h, 20 + k) for k in range(n)])
        if n == 2:
            maps[1] = maps[1, ::-1]   # (comb and spiral take no seed: the second frame upside down)
        with api.Context(w, h, 1, n) as ctx:
            for conn in (4, 8):
                _, got = _call(ctx, maps, conn, w * h + 1, w + 3, base_off=1, label_pad=8, what=f"{kind} {w}x{h} n={n} c={conn}")
                assert kind == "random0.3" or (int(got[0]) == 2 and (h > 1000 or int(got[1]) == 2))
                assert kind != "random0.3" or int(got.min()) > 500   # (604 .. 4431: roots in every chunk, behind the carries too)


def test_chunks_of_nine_rows_straddle_the_tiles():
    """5 x 1030, 64 frames: 65,920 rows in the call, so hist_chunk_rows gives 9 and a frame has 115 chunks whose borders fall on
    no multiple of the 32 rows of a tile but 288, 576 and 864; k_ccl_scan carries once per frame."""
    w, h, n = 5, 1030, 64
    assert (h * n + 8191) // 8192 == 9 and (h + 8) // 9 == 115
    maps = np.stack([_content("random0.5", w, h, 300 + k) for k in range(n)])
    with api.Context(w, h, 1, n) as ctx:
        for conn in (4, 8):
            _, got = _call(ctx, maps, conn, 1200, w + 3, (w + 3) * h + 5, base_off=2, label_pad=4, label_gap=12, what=f"chunk_rows 9, c={conn}")
            assert 100 < int(got.min()) and int(got.max()) < 1200   # nothing is cut


def test_more_rows_of_statistics_than_threads():
    """A 1024 x 514 checkerboard at connectivity 4: N = 263,169 rows of statistics, 1,025 more than the 262,144 threads k_ccl_rows
    and k_ccl_finish have per frame, so the last rows are the second trip of their stride.  Capacity N: the whole trip; 262,144 +
    77: a capacity that cuts inside it; 262,144: no second trip.  _call checks that each slot's tail stays canary."""
    w, h = 1024, 514
    want = R.checkerboard4(w, h)
    n = want[1]
    assert n == 263169 > ROW_THREADS
    maps = _content("checkerboard", w, h)[None]
    want = (want[0][None], np.array([n], np.uint32), [want[2]], [want[3]])
    with api.Context(w, h, 1, 1) as ctx:
        for cap in (n, ROW_THREADS + 77, ROW_THREADS):
            _call(ctx, maps, 4, cap, what=f"checkerboard, capacity {cap}", want=want)


@pytest.mark.parametrize("kind", ["full", "empty", "left half"])
def test_coordinate_sums_beyond_32_bits(kind):
    """2100 x 2100: the sums of x and of y of the full frame's component, and of the empty frame's background, are 4,628,295,000 >
    2^32 -- through the atomicAdd on 64 bits in the one case, through the registers and shfl_xor64 in the other.  A sum narrowed to
    32 bits anywhere gives another centroid; the centroids are compared in their bits."""
    w = h = 2100
    assert w * h * (h - 1) // 2 == 4628295000 > 1 << 32
    x1 = {"full": w, "empty": 0, "left half": w // 2}[kind]
    want = R.columns(w, h, x1)
    maps = np.zeros((1, h, w), np.uint8)
    maps[0, :, :x1] = 255
    conn = 4 if kind == "empty" else 8
    with api.Context(w, h, 1, 1) as ctx:
        _call(ctx, maps, conn, 3, what=f"2100 x 2100 {kind}", want=(want[0][None], np.array([want[1]], np.uint32), [want[2]], [want[3]]))
