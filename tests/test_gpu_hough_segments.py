"""hc_hough_segments_device (k_seg_count, k_seg_scan, k_seg_emit) on the MI355X: segment counts and segments equal, value for value
and in order, to the numpy restatement tests/hough_segments_ref.py.  Every call writes its counts between two guard words and its
segments into a buffer pre-filled with a canary with guard space on both sides -- everything but the first min(count,
seg_capacity) segments of each frame's slot must still hold the canary -- and reads a map (inside an arena of 255s, which would
add edges if a reader strayed) and lines that must come back unchanged.

The shapes are the smallest at which the paths differ: walks shorter than, equal to, one more than and a few chunks of a wave on
both axes, and walks of more than 256 and more than 512 steps, where the kernels' trips of four chunks repeat and skip.

No vacuous passes: each parametrised case asserts, on the restatement alone, that its input has a kept segment, a group dropped
by min_length and a walk cut by max_gap (a frame of one pixel can hold neither of the last two and has a test of its own)."""
import contextlib
import math

import numpy as np
import pytest

import hough_ref as R
import hough_segments_ref as S
import view_arena as VA
from cudacam_amd import api, synth

pytestmark = pytest.mark.gpu

CANARY = -0x5A5A5A5B
GUARD = 64   # int32 words: 256 bytes, so the slots behind it keep the allocation's 16-byte alignment
PI = math.pi
GEO12 = (1.0, PI / 12, 0.0, PI)       # twelve angles, 45 and 135 degrees (the x-major / y-major switch) among them
GEO7 = (2.0, PI / 7, 0.2, 2.9)        # six angles off every axis, rho 2
AXES = (1.0, PI / 2, 0.0, PI)         # two angles: x = rho (a step per row) and y = rho (a step per column)
SIZES = [(7, 5), (61, 33), (64, 48), (65, 64), (130, 67), (250, 200), (300, 40), (40, 300)]


def _hand_lines(w, h, geo):
    """Lines independent of any vote: every angle of the table with a rho through the frame's middle on the accumulator's grid,
    one off it, and a negative one; then lines that must yield nothing."""
    rho = geo[0]
    tt = R.tables(w, h, *geo)[2]
    lines = []
    for n, th in enumerate(tt):
        mid = (w / 2) * math.cos(float(th)) + (h / 2) * math.sin(float(th))
        lines += [(round(mid / rho) * rho, th, 9), (mid + 0.37 + 0.11 * n, th, 8), (-3.0 * rho, th, 7), (1.25, th, 6)]
    lines += [(3.0, np.float32(0.123), 5), (3.0, np.float32(math.nan), 5), (math.nan, tt[0], 5), (math.inf, tt[-1], 5), (-math.inf, tt[0], 5),
              (1e30, tt[0], 5), (-1e9, tt[-1], 5), (float(4 * (w + h)), tt[len(tt) // 2], 5), (3.0, np.nextafter(tt[0], np.float32(9)), 5)]
    return np.array(lines, np.float32)


def _drawn(w, h, geo, lines, min_length, max_gap, seed, noise=0.0):
    """A map of runs along the walks of every fourth of `lines` (_hand_lines: the one through the middle, at every angle): runs
    joined by gaps of max_gap, cut by gaps of max_gap + 1, runs just long enough for min_length and one step too short, single
    pixels; `noise`: that share of random edges on top."""
    rng = np.random.default_rng(seed)
    m = np.zeros((h, w), np.uint8)
    tt = R.tables(w, h, *geo)[2]
    for k in range(0, len(lines), 4):
        hit = np.flatnonzero(tt.view(np.uint32) == lines[k, 1:2].view(np.uint32))
        if len(hit) == 0 or not np.isfinite(lines[k, 0]):
            continue
        small = max(w, h) < 20   # a short walk: a pixel, a cut, then the run that is kept
        t, runs = (0 if small else int(rng.integers(0, 3))), ([1, min_length + 1, 1] if small else [min_length + 1, 4, min_length, 2, min_length + 3, 1])
        for j in range(64):
            run = runs[j % len(runs)]
            S.draw(m, w, h, *geo, int(hit[0]), float(lines[k, 0]), t, t + run - 1)
            t += run + max_gap + (j % 3 != 2)   # a gap of max_gap (joins) after every third run, of max_gap + 1 (cuts) after the others
            if t >= max(w, h):
                break
    if noise:
        m[rng.random((h, w)) < noise] = 255
    return m


def _upload(maps, lines, line_counts, seg_capacity, pitch=None, frame_stride=None, base_off=0):
    """The buffers of one call: the maps inside an arena of 255s, lines [n][lcap][3] and their counts, the segment counts between
    two guard words and the segment slots between guards, pre-filled with the canary."""
    import torch
    n, h, w = maps.shape
    arena, off = VA.make_input(maps, pitch or w, frame_stride, base_off, fill="ff")
    g = VA.input_geometry(maps, pitch or w, frame_stride, base_off)
    lines = np.ascontiguousarray(lines, np.float32)
    return dict(n=n, w=w, h=h, maps=maps, arena=arena, off=off, g=g, lines=lines, lcounts=np.asarray(line_counts, np.uint32), lcap=lines.shape[1], cap=seg_capacity,
                d_arena=torch.from_numpy(arena).cuda(), d_lines=torch.from_numpy(lines.view(np.int32)).cuda(),
                d_lc=torch.from_numpy(np.asarray(line_counts, np.uint32).view(np.int32)).cuda(),
                counts=torch.full((n + 2,), CANARY, dtype=torch.int32, device="cuda"),
                segs=torch.full((2 * GUARD + 4 * n * seg_capacity,), CANARY, dtype=torch.int32, device="cuda"))


def _queue(ctx, b, geo, min_length, max_gap, null_segs=False):
    ctx.hough_segments_device(b["d_arena"].data_ptr() + b["off"], b["g"].pitch, b["g"].frame_stride, b["d_lines"].data_ptr(), b["d_lc"].data_ptr(), b["lcap"], b["n"],
                              *geo, min_length, max_gap, b["counts"].data_ptr() + 4, None if null_segs else b["segs"].data_ptr() + 4 * GUARD, b["cap"])


def _check(b, geo, min_length, max_gap, what="", stats=None):
    """What a call left behind (the context has been synchronised), compared with the restatement.  Returns (counts, segments)."""
    n, cap = b["n"], b["cap"]
    assert np.array_equal(b["d_arena"].cpu().numpy(), b["arena"]), f"{what}: the map or the bytes around it were written"
    assert np.array_equal(b["d_lines"].cpu().numpy(), b["lines"].view(np.int32)) and np.array_equal(b["d_lc"].cpu().numpy().view(np.uint32), b["lcounts"]), f"{what}: the lines were written"
    c = b["counts"].cpu().numpy()
    assert c[0] == CANARY and c[-1] == CANARY, f"{what}: a word beside d_seg_counts was written"
    got_counts = c[1:-1].view(np.uint32)
    walked = [b["lines"][f, :min(int(b["lcounts"][f]), b["lcap"])] for f in range(n)]
    want_counts, want = S.segments_batch(b["maps"], walked, b["w"], b["h"], *geo, min_length, max_gap, cap, stats)
    assert got_counts.tolist() == want_counts.tolist(), f"{what}: counts {got_counts.tolist()} != {want_counts.tolist()}"
    s = b["segs"].cpu().numpy()
    assert (s[:GUARD] == CANARY).all() and (s[len(s) - GUARD:] == CANARY).all(), f"{what}: the guard around d_segs was written"
    slots = s[GUARD:len(s) - GUARD].reshape(n, cap, 4)
    for f in range(n):
        k = len(want[f])
        assert k == min(int(want_counts[f]), cap)
        if not np.array_equal(slots[f, :k], want[f]):
            bad = np.flatnonzero((slots[f, :k] != want[f]).any(axis=1))
            raise AssertionError(f"{what}: frame {f}: {len(bad)} of {k} segments differ; first (index, hip, numpy): "
                                 f"{[(int(i), slots[f, i].tolist(), want[f][i].tolist()) for i in bad[:6]]}")
        assert (slots[f, k:] == CANARY).all(), f"{what}: frame {f}: the slot was written behind its {k} segments"
    return got_counts, want


def _call(ctx, maps, lines, line_counts, geo, min_length, max_gap, seg_capacity, null_segs=False, what="", stats=None, **view):
    import torch
    b = _upload(maps, lines, line_counts, seg_capacity, **view)
    torch.cuda.synchronize()
    _queue(ctx, b, geo, min_length, max_gap, null_segs)
    ctx.sync()
    return _check(b, geo, min_length, max_gap, what, stats)


def _not_vacuous(stats, what):
    assert stats["kept"] > 0 and stats["dropped"] > 0 and stats["cuts"] > 0, f"{what}: a vacuous input: {stats}"


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_size_and_hand_made_lines(size):
    w, h = size
    min_length, max_gap = (3, 1) if min(w, h) < 10 else (6, 2)
    for gi, geo in enumerate((GEO12, GEO7, AXES)):
        lines = _hand_lines(w, h, geo)
        maps = np.stack([_drawn(w, h, geo, lines, min_length, max_gap, 10 * gi), _drawn(w, h, geo, lines, min_length, max_gap, 10 * gi + 1, noise=0.05),
                         np.full((h, w), 255, np.uint8), np.zeros((h, w), np.uint8), _drawn(w, h, geo, lines, min_length, max_gap, 10 * gi + 2, noise=0.3)])
        n = len(maps)
        batch = np.repeat(lines[None], n, axis=0)
        stats = {}
        S.segments_of(maps[0], lines, w, h, *geo, min_length, max_gap, None, stats)   # the drawn map alone
        _not_vacuous(stats, f"{w}x{h} geo {gi}")
        with api.Context(w, h, 1, n, api.MODE_O if gi % 2 else api.MODE_R) as ctx:   # either mode
            t = f"{w}x{h} geo {gi}"
            counts, _ = _call(ctx, maps, batch, [len(lines)] * n, geo, min_length, max_gap, 4 * len(lines) * max(w, h) // 2, what=t)
            assert counts[3] == 0 and counts[0] > 0 and counts[2] > 0
            _call(ctx, maps, batch, [len(lines)] * n, geo, 0, 0, 64, what=t + " every pixel a segment, cut lists")
            _call(ctx, maps, batch, [len(lines)] * n, geo, min_length, max(w, h), 8, what=t + " no gap cuts")
            _call(ctx, maps[:1], batch[:1], [len(lines)], geo, min_length, max_gap, 0, null_segs=True, what=t + " counts only")


def test_a_frame_of_one_pixel():
    """1 x 1: every walk has one step.  The pixel is a segment of length 0: kept at min_length 0, dropped at 1; nothing can be cut."""
    lines = _hand_lines(1, 1, GEO12)
    maps = np.array([[[255]], [[0]]], np.uint8)
    batch = np.repeat(lines[None], 2, axis=0)
    with api.Context(1, 1, 1, 2) as ctx:
        counts, want = _call(ctx, maps, batch, [len(lines)] * 2, GEO12, 0, 0, 100, what="1x1")
        assert counts[0] > 0 and counts[1] == 0 and (want[0] == 0).all()
        counts, _ = _call(ctx, maps, batch, [len(lines)] * 2, GEO12, 1, 0, 100, what="1x1, min_length 1")
        assert counts.tolist() == [0, 0]


@pytest.mark.parametrize("column", [False, True], ids=["rows", "columns"])
def test_groups_at_lanes_0_and_63_and_across_chunks(column):
    """Walks along one row (or, transposed, one column) of 600 steps: groups that start, end and bridge at lanes 0 and 63, at the
    chunk boundaries 64, 128, 192, at the boundary of a trip of four chunks (256, 512), across a whole empty chunk and a whole empty
    trip, and up to the last step."""
    L = 600
    layouts = [
        [(0, 0), (63, 63), (64, 64), (127, 128), (190, 200), (255, 256), (300, 511), (512, 512), (599, 599)],
        [(0, 63), (64, 127), (129, 140), (250, 260), (510, 514), (580, 599)],
        [(5, 5), (590, 590)],                      # joined only by a max_gap of 584 and more: across empty chunks and an empty trip
        [(60, 70), (120, 130), (255, 255), (257, 257), (319, 320), (383, 384), (447, 448)],
        [(0, 599)],
        [(63, 63)], [(64, 64)], [(256, 256)], [(0, 0)],
    ]
    n = len(layouts)
    rows = np.zeros((n, 3, L), np.uint8)
    for f, runs in enumerate(layouts):
        for a, b in runs:
            rows[f, 1, a:b + 1] = 255
    maps = np.ascontiguousarray(rows.transpose(0, 2, 1)) if column else rows
    w, h = (3, L) if column else (L, 3)
    tt = R.tables(w, h, *AXES)[2]
    lines = np.array([(1.0, tt[0 if column else 1], 1), (0.0, tt[0 if column else 1], 1), (2.0, tt[0 if column else 1], 1)], np.float32)
    batch = np.repeat(lines[None], n, axis=0)
    with api.Context(w, h, 1, n) as ctx:
        for min_length, max_gap in ((0, 0), (0, 1), (1, 0), (5, 3), (10, 9), (0, 583), (0, 584), (0, 10 ** 9), (2, 55), (599, 0), (600, 0)):
            stats = {}
            _call(ctx, maps, batch, [3] * n, AXES, min_length, max_gap, 40, what=f"min_length {min_length} max_gap {max_gap}", stats=stats)
            if (min_length, max_gap) == (5, 3):
                _not_vacuous(stats, "chunk boundaries")
        counts, want = _call(ctx, maps, batch, [3] * n, AXES, 0, 584, 40, what="a gap of 584 joins")
        e = [1, 5, 1, 590] if column else [5, 1, 590, 1]
        assert counts[2] == 1 and want[2].tolist() == [e]
        counts, _ = _call(ctx, maps, batch, [3] * n, AXES, 0, 583, 40, what="a gap of 583 cuts")
        assert counts[2] == 2


def test_segment_capacities_around_the_count():
    w, h, min_length, max_gap = 64, 48, 6, 2
    lines = _hand_lines(w, h, GEO12)
    maps = np.stack([_drawn(w, h, GEO12, lines, min_length, max_gap, 3), _drawn(w, h, GEO12, lines, min_length, max_gap, 4, noise=0.05)])
    batch = np.repeat(lines[None], 2, axis=0)
    stats = {}
    (c0, _), (c1, _) = (S.segments_of(m, lines, w, h, *GEO12, min_length, max_gap, None, stats) for m in maps)
    _not_vacuous(stats, "capacities")
    assert c0 > 2 and c1 > 2 and c0 != c1
    with api.Context(w, h, 1, 2) as ctx:
        _call(ctx, maps, batch, [len(lines)] * 2, GEO12, min_length, max_gap, 0, null_segs=True, what="capacity 0, null")
        _call(ctx, maps, batch, [len(lines)] * 2, GEO12, min_length, max_gap, 0, what="capacity 0, a pointer")
        for cap in sorted({1, c0 - 1, c0, c0 + 1, c1 - 1, c1, c1 + 1}):
            _call(ctx, maps, batch, [len(lines)] * 2, GEO12, min_length, max_gap, cap, what=f"capacity {cap}")


def test_nine_frames_with_different_line_counts():
    """d_line_counts 0, 1, below, at and above line_capacity (the walk stops at the capacity), each frame with lines of its own."""
    w, h, min_length, max_gap, n = 61, 33, 6, 2, 9
    lines = _hand_lines(w, h, GEO12)
    lcap = 20
    rng = np.random.default_rng(5)
    batch = np.stack([lines[rng.permutation(len(lines))[:lcap]] for _ in range(n)])
    maps = np.stack([_drawn(w, h, GEO12, lines, min_length, max_gap, 20 + f, noise=0.05 * (f % 3)) for f in range(n)])
    lcounts = [0, 1, 19, 20, 21, 1000, 0xFFFFFFFF, 7, 0]
    stats = {}
    with api.Context(w, h, 1, n) as ctx:
        counts, _ = _call(ctx, maps, batch, lcounts, GEO12, min_length, max_gap, 200, what="nine frames", stats=stats)
        _not_vacuous(stats, "nine frames")
        assert counts[0] == 0 and counts[8] == 0 and counts[3] > 0 and len(set(counts.tolist())) > 4
        _call(ctx, maps[:4], batch[:4], lcounts[:4], GEO12, min_length, max_gap, 5, what="four of them, cut lists")


def test_a_pitched_offset_roi_view():
    """Odd base, odd pitch, a frame stride that is no multiple of the pitch: every byte around the ROI is 255."""
    w, h, min_length, max_gap, n = 65, 64, 6, 2, 3
    lines = _hand_lines(w, h, GEO12)
    maps = np.stack([_drawn(w, h, GEO12, lines, min_length, max_gap, 30 + f, noise=0.03 * f) for f in range(n)])
    batch = np.repeat(lines[None], n, axis=0)
    stats = {}
    with api.Context(w, h, 1, n) as ctx:
        tight, _ = _call(ctx, maps, batch, [len(lines)] * n, GEO12, min_length, max_gap, 300, what="tight", stats=stats)
        _not_vacuous(stats, "views")
        for pitch, extra, base in ((67, 0, 1), (131, 77, 13), (65, 1, 3)):
            got, _ = _call(ctx, maps, batch, [len(lines)] * n, GEO12, min_length, max_gap, 300, what=f"pitch {pitch} base {base}", pitch=pitch, frame_stride=pitch * h + extra, base_off=base)
            assert got.tolist() == tight.tolist()


def test_tables_remade_when_the_geometry_changes():
    """Calls on one context with other geometry (fewer angles in the old allocation, then more than it holds), then the first again;
    and four calls with no synchronisation between them, each finding the one before still queued when it replaces the tables."""
    import torch
    w, h, min_length, max_gap = 64, 48, 6, 2
    geos = [GEO12, GEO7, (1.0, PI / 180, 0.0, PI), GEO12]
    per = []
    for k, geo in enumerate(geos):
        lines = _hand_lines(w, h, geo)
        maps = np.stack([_drawn(w, h, geo, lines, min_length, max_gap, 40 + k, noise=0.02)])
        stats = {}
        S.segments_of(maps[0], lines, w, h, *geo, min_length, max_gap, None, stats)
        _not_vacuous(stats, f"tables {k}")
        per.append((geo, maps, lines[None]))
    with api.Context(w, h, 1, 1) as ctx:
        for k, (geo, maps, batch) in enumerate(per):
            counts, _ = _call(ctx, maps, batch, [batch.shape[1]], geo, min_length, max_gap, 2000, what=f"call {k}")
            assert counts[0] > 0
        bufs = [_upload(maps, batch, [batch.shape[1]], 2000) for _, maps, batch in per]
        torch.cuda.synchronize()
        for b, (geo, _, _) in zip(bufs, per):
            _queue(ctx, b, geo, min_length, max_gap)
        ctx.sync()
        for k, (b, (geo, _, _)) in enumerate(zip(bufs, per)):
            _check(b, geo, min_length, max_gap, f"queued call {k}")


def _chain_want(maps, w, h, rho, theta, threshold, min_length, max_gap):
    """The restatements applied one after the other to the maps a chain returned: (line counts, segment counts, segments)."""
    lcounts, lines = R.hough_lines_batch([R.points_of(m) for m in maps], w, h, rho, theta, threshold)
    scounts, segs = S.segments_batch(maps, lines, w, h, rho, theta, 0.0, R.PI, min_length, max_gap)
    return lcounts, scounts, segs


def _same(counts, segs, want_counts, want):
    assert counts.dtype == np.uint32 and counts.tolist() == want_counts.tolist()
    assert len(segs) == len(want) and all(a.dtype == np.int32 and a.shape == b.shape and np.array_equal(a, b) for a, b in zip(segs, want))


@pytest.mark.parametrize("pipelined", [False, True])
def test_hough_segments_and_canny_segments(pipelined):
    w, h, n = 250, 200, 3
    frames = np.stack([synth.natural(w, h, 40 + k) for k in range(n)])
    args = dict(rho=1.0, theta=PI / 180, threshold=25, min_length=12, max_gap=3)
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        if pipelined:
            ctx.set_option(api.OPT_PIPELINE, 1)
        maps = ctx.canny(frames, 50, 150)
        lcounts, want_counts, want = _chain_want(maps, w, h, *args.values())
        assert lcounts.min() > 0 and want_counts.min() > 0
        stats = {}
        S.segments_batch(maps, R.hough_lines_batch([R.points_of(m) for m in maps], w, h, 1.0, PI / 180, 25)[1], w, h, 1.0, PI / 180, 0.0, R.PI, 12, 3, None, stats)
        _not_vacuous(stats, "the chain")
        _same(*ctx.hough_segments(maps, **args), want_counts, want)   # the counts passes size every buffer
        import torch
        counts, segs = ctx.hough_segments(torch.from_numpy(maps).cuda(), max_segments=2, **args)   # torch maps, cut segment lists
        _same(counts, segs, want_counts, [s[:2] for s in want])
        cut_lines = [l[:3] for l in R.hough_lines_batch([R.points_of(m) for m in maps[:1]], w, h, 1.0, PI / 180, 25)[1]]
        _same(*ctx.hough_segments(maps[0], max_lines=3, **args), *S.segments_batch(maps[:1], cut_lines, w, h, 1.0, PI / 180, 0.0, R.PI, 12, 3))   # one map, cut line lists
        counts, segs = ctx.hough_segments(maps, max_lines=0, **args)
        assert counts.tolist() == [0] * n and all(s.shape == (0, 4) for s in segs)
        for blur in (None, (5, 1.2)):
            got_maps, counts, segs = ctx.canny_segments(frames, 50, 150, blur=blur, **args)
            if blur is None:
                assert np.array_equal(got_maps, maps)
            _, wc, ws = _chain_want(got_maps, w, h, *args.values())
            _same(counts, segs, wc, ws)


@pytest.mark.parametrize("own_stream", [True, False], ids=["context stream", "torch stream"])
def test_pipelined_runs_in_flight_on_rotated_outputs(own_stream):
    """Two pipelined runs into rotating outputs, then points, lines and segments of the first output queued behind them with no
    synchronisation: the segments are those of the final maps, not of the provisional ones.  Once on the context's own stream, once
    through hc_set_stream on torch's current stream."""
    import torch
    w, h, n = 250, 200, 4
    a = np.stack([synth.natural(w, h, 70 + k) for k in range(n)])
    b = np.stack([synth.natural(w, h, 90 + k) for k in range(n)])
    d_in = [torch.from_numpy(v).cuda() for v in (a, b)]
    outs = [torch.zeros((n, h, w), dtype=torch.uint8, device="cuda") for _ in range(2)]
    pcap, lcap, scap = w * h // 4, 64, 400
    pts = torch.empty((n, pcap, 2), dtype=torch.int32, device="cuda")
    pc = torch.empty((n,), dtype=torch.int32, device="cuda")
    lines = torch.empty((n, lcap, 3), dtype=torch.float32, device="cuda")
    lc = torch.empty((n,), dtype=torch.int32, device="cuda")
    counts = torch.full((n + 2,), CANARY, dtype=torch.int32, device="cuda")
    segs = torch.full((2 * GUARD + 4 * n * scap,), CANARY, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    geo = (1.0, PI / 180, 0.0, PI)
    side = torch.cuda.Stream()
    with api.Context(w, h, 1, n, api.MODE_R) as ctx, (contextlib.nullcontext() if own_stream else torch.cuda.stream(side)):
        ctx.set_option(api.OPT_PIPELINE, 1)
        if not own_stream:
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        for r in range(2):
            ctx.run_device(d_in[r].data_ptr(), w, w * h, outs[r].data_ptr(), w, w * h, n)
        ctx.edge_points_device(outs[0].data_ptr(), w, w * h, n, pc.data_ptr(), pts.data_ptr(), pcap)
        ctx.hough_lines_device(pts.data_ptr(), pc.data_ptr(), pcap, n, 1.0, PI / 180, 25, 0.0, PI, lc.data_ptr(), lines.data_ptr(), lcap)
        ctx.hough_segments_device(outs[0].data_ptr(), w, w * h, lines.data_ptr(), lc.data_ptr(), lcap, n, *geo, 12, 3, counts.data_ptr() + 4, segs.data_ptr() + 4 * GUARD, scap)
        ctx.sync()
        torch.cuda.synchronize()
        maps = outs[0].cpu().numpy()
        assert maps.any()
        got_lc, got_lines = lc.cpu().numpy().view(np.uint32), lines.cpu().numpy()
        walked = [got_lines[f, :min(int(got_lc[f]), lcap)] for f in range(n)]
        want_lc, want_lines = R.hough_lines_batch([R.points_of(m) for m in maps], w, h, 1.0, PI / 180, 25, capacity=lcap)
        assert got_lc.tolist() == want_lc.tolist() and all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(walked, want_lines))
        stats = {}
        want_counts, want = S.segments_batch(maps, walked, w, h, *geo, 12, 3, scap, stats)
        _not_vacuous(stats, "pipelined")
        c = counts.cpu().numpy()
        assert c[0] == CANARY and c[-1] == CANARY and c[1:-1].view(np.uint32).tolist() == want_counts.tolist()
        s = segs.cpu().numpy()
        assert (s[:GUARD] == CANARY).all() and (s[len(s) - GUARD:] == CANARY).all()
        slots = s[GUARD:len(s) - GUARD].reshape(n, scap, 4)
        for f in range(n):
            assert np.array_equal(slots[f, :len(want[f])], want[f]) and (slots[f, len(want[f]):] == CANARY).all(), f
        if not own_stream:
            ctx.use_own_stream()


def test_not_a_run():
    w, h, n = 250, 65, 2
    frames = np.stack([synth.natural(w, h, 60 + k) for k in range(n)])
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        maps = ctx.canny(frames, 50, 150)
        before = (ctx.hysteresis_schedule(), ctx.last_run_info(), ctx.pipeline_slots_in_use(), ctx.hysteresis_totals(), ctx.hysteresis_info())
        lines = _hand_lines(w, h, GEO12)
        batch = np.repeat(lines[None], n, axis=0)
        counts, _ = _call(ctx, maps, batch, [len(lines)] * n, GEO12, 4, 2, 500, what="after a run")
        assert counts.min() > 0
        assert before == (ctx.hysteresis_schedule(), ctx.last_run_info(), ctx.pipeline_slots_in_use(), ctx.hysteresis_totals(), ctx.hysteresis_info())


def test_argument_errors():
    import torch
    w, h = 16, 8
    maps = torch.full((2, h, w), 255, dtype=torch.uint8, device="cuda")
    tt = R.tables(w, h, 1.0, PI / 180)[2]
    lines = torch.from_numpy(np.array([[(3.0, tt[90], 1)] * 4] * 2, np.float32)).cuda()
    lc = torch.full((2,), 4, dtype=torch.int32, device="cuda")
    counts = torch.full((4,), CANARY, dtype=torch.int32, device="cuda")
    segs = torch.full((2 * 8 * 4 + 8,), CANARY, dtype=torch.int32, device="cuda")
    m, l, q, c, s = maps.data_ptr(), lines.data_ptr(), lc.data_ptr(), counts.data_ptr(), segs.data_ptr()
    torch.cuda.synchronize()
    T = PI / 180
    inf, nan = math.inf, math.nan
    with api.Context(w, h, 1, 2) as ctx:
        good = (m, w, w * h, l, q, 4, 1, 1.0, T, 0.0, PI, 2, 1, c, s, 8)
        names = ("map", "pitch", "fs", "lines", "lcounts", "lcap", "n", "rho", "theta", "lo", "hi", "min_length", "max_gap", "counts", "segs", "scap")

        def change(**kw):
            return tuple(kw.get(k, v) for k, v in zip(names, good))
        bad = [change(map=0), change(lines=0), change(lcounts=0), change(counts=0), change(segs=0), change(lines=l + 2), change(lcounts=q + 1), change(counts=c + 2),
               change(segs=s + 4), change(segs=s + 8), change(segs=s + 1, scap=0), change(min_length=-1), change(max_gap=-1), change(n=0), change(n=-1), change(n=3),
               change(pitch=w - 1), change(n=2, fs=w * h - 1), change(pitch=(1 << 32) // h + 1), change(lcap=0), change(lcap=(1 << 64) // 12 + 1), change(lcap=(1 << 64) // 4 + 1),
               change(scap=(1 << 64) // 16 + 1), change(lcap=1 << 31), change(hi=-0.5), change(lo=1.0, hi=0.5), change(rho=1e-4), change(theta=1e-9)]
        bad += [change(rho=v) for v in (0.0, -1.0, inf, nan)] + [change(theta=v) for v in (0.0, -1.0, inf, nan)]
        bad += [change(lo=v) for v in (inf, -inf, nan)] + [change(hi=v) for v in (inf, nan)]
        for args in bad:
            with pytest.raises(api.HipCannyError, match="error -1"):
                ctx.hough_segments_device(*args)
            assert "hc_hough_segments_device" in api.last_error()
        assert api.load_library().hc_hough_segments_device(None, *good) == -1   # ctx null
        ctx.sync()
        torch.cuda.synchronize()
        assert (counts.cpu().numpy() == CANARY).all() and (segs.cpu().numpy() == CANARY).all()
        ctx.hough_segments_device(*change(n=2))   # the same buffers are fine for a good call: row 3 of an all-edge map, four times per frame
        ctx.sync()
        assert counts.cpu().numpy()[:2].tolist() == [4, 4] and segs.cpu().numpy()[:16].reshape(4, 4).tolist() == [[0, 3, w - 1, 3]] * 4
