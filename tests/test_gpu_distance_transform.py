"""hc_distance_transform_device (dist.hip) on the MI355X: squared distances (int32), their roots (as float32 bit patterns) and the
nearest feature pixel equal, value for value, to the brute-force restatement tests/dist_ref.py.

Every call reads its maps from a guarded arena (tests/view_arena.py) that must come back unchanged and writes its planes into
canary-filled pitched arenas in which only [row, row + 4 W) of each row may change.

The shapes are the smallest at which the paths differ: k_dt_cols has one column per lane and 64 lanes per workgroup, k_dt_rows 256
threads that stride over the row and 4 rows per workgroup, the column pass loads 8 rows ahead; 16384 columns fill the LDS row."""
import numpy as np
import pytest

import dist_ref as R
import view_arena as VA
from cudacam_amd import api, synth

pytestmark = pytest.mark.gpu

COL_THREADS, ROW_THREADS, ROWS, LOOKAHEAD = 64, 256, 4, 8   # canny_params.h: DT_COL_THREADS, DT_ROW_THREADS, DT_ROWS, DT_LOOKAHEAD
WIDTHS = (1, 2, 3, 63, 64, 65, 2 * COL_THREADS + 1, ROW_THREADS - 1, ROW_THREADS, ROW_THREADS + 1, 2 * ROW_THREADS + 1)
HEIGHTS = (1, 2, 3, ROWS, ROWS + 1, LOOKAHEAD - 1, LOOKAHEAD, LOOKAHEAD + 1)
SQ, F32 = api.DT_SQUARED_I32, api.DT_F32
NZ, ZERO = api.DT_TO_NONZERO, api.DT_TO_ZERO

_REF = {}


def _ref(maps, target):
    """The restatement of a batch, computed once per (content, target) and shared; never modified."""
    key = (maps.shape, maps.tobytes(), target)
    if key not in _REF:
        _REF[key] = R.distance_transform(maps, target)
    return _REF[key]


def _content(kind, w, h, seed=0):
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), np.uint8)
    if kind == "empty":
        return m
    if kind == "full":
        return m + 255
    if kind in ("nw", "ne", "sw", "se", "centre"):
        y, x = {"nw": (0, 0), "ne": (0, w - 1), "sw": (h - 1, 0), "se": (h - 1, w - 1), "centre": (h // 2, w // 2)}[kind]
        m[y, x] = 255
        return m
    if kind == "row":
        m[h // 2] = 255
        return m
    if kind == "column":
        m[:, w // 3] = 255
        return m
    if kind == "ends":      # the tie along the row: features at both ends, the middle goes to x' = 0
        m[:, 0] = m[:, w - 1] = 255
        return m
    if kind == "top-bottom":   # the tie between above and below
        m[0] = m[h - 1] = 255
        return m
    if kind == "345":       # a straight 5 against 3-4-5 on both sides, every 16 columns
        m[0, 5::16] = 255
        m[min(4, h - 1), 2::8] = 255
        return m
    if kind == "checkerboard":
        return np.where((xx + yy) % 2 == 0, 255, 0).astype(np.uint8)
    if kind == "sparse":    # 1 %
        return np.where(np.random.default_rng(500 + seed).random((h, w)) < 0.01, 255, 0).astype(np.uint8)
    if kind == "mixed":     # only the values 0 / 1 / 128
        return np.random.default_rng(600 + seed).choice(np.array([0, 0, 0, 0, 1, 128], np.uint8), size=(h, w))
    if kind.startswith("random"):
        return np.where(np.random.default_rng(700 + seed).random((h, w)) < float(kind[6:]), 255, 0).astype(np.uint8)
    raise ValueError(kind)


def _call(ctx, maps, target, dist_type, nearest=True, pitch=None, frame_stride=None, base_off=0, pad=(0, 0), gap=(0, 0), off=(0, 0), fill="ff", what=""):
    """One call on `maps` (n, H, W) in guarded arenas; pad / gap / off: of the distance and of the nearest view, in bytes."""
    import torch
    n, h, w = maps.shape
    pitch = w if pitch is None else pitch
    arena, moff = VA.make_input(maps, pitch, frame_stride, base_off, fill, seed=w + h)
    g = VA.input_geometry(maps, pitch, frame_stride, base_off)
    planes = []
    for k in range(2):
        p = 4 * w + pad[k]
        a, pg = VA.make_output(n, h, 4 * w, p, p * h + gap[k], off[k], lead=VA.round_up(p + 64, 4), seed=w + k)
        planes.append((a, pg, torch.from_numpy(a).cuda()))
    d = torch.from_numpy(arena).cuda()
    torch.cuda.synchronize()
    (da, dg, dd), (na, ng, dn) = planes
    assert (dd.data_ptr() + dg.offset) % 4 == 0 and (dn.data_ptr() + ng.offset) % 4 == 0
    ctx.distance_transform_device(d.data_ptr() + moff, pitch, g.frame_stride, n, target, dist_type, dd.data_ptr() + dg.offset, dg.pitch, dg.frame_stride,
                                  dn.data_ptr() + ng.offset if nearest else None, ng.pitch if nearest else 0, ng.frame_stride if nearest else 0)
    ctx.sync()
    d2, near = _ref(maps, target)
    what = f"{what} {w}x{h} n={n} target={target} type={dist_type} nearest={nearest}"
    assert np.array_equal(d.cpu().numpy(), arena), f"{what}: the map arena was written"
    VA.check_output(dd.cpu().numpy(), da, dg, d2 if dist_type == SQ else R.root_f32(d2), what=f"{what}: distances")
    if nearest:
        VA.check_output(dn.cpu().numpy(), na, ng, near, what=f"{what}: nearest")
    else:
        assert np.array_equal(dn.cpu().numpy(), na), f"{what}: an arena that was not passed was written"
    return d2, near


def _varied(ctx, maps, what):
    """Eight calls: both targets, both types, with and without the nearest plane; map offsets 0..3, tight and padded pitches on all
    three views, gaps between the frames, the planes as ROIs at word offsets."""
    n, h, w = maps.shape
    for c in range(8):
        target, dist_type, nearest = c & 1, (c >> 1) & 1, c != 5 and c != 2
        if c in (0, 4):
            _call(ctx, maps, target, dist_type, nearest, what=f"{what} tight")
        else:
            mp = w + (0, 3, 1, 13)[c % 4]
            _call(ctx, maps, target, dist_type, nearest, mp, mp * h + (c if n > 1 else 0), base_off=c & 3, pad=(4 * (c % 3), 4 * ((c + 1) % 3)), gap=(8 * (c & 2), 4 * c),
                  off=(4 * (c & 3), 4 * (c % 3)), fill=("ff", "random")[c % 2], what=f"{what} views {c}")


@pytest.mark.parametrize("w", WIDTHS)
def test_every_width_and_height(w):
    for h in HEIGHTS:
        kinds = ("random0.3", "sparse", ("nw", "se", "centre", "ne", "sw")[(w + h) % 5])
        maps = np.stack([_content(k, w, h, 10 * w + h + i) for i, k in enumerate(kinds)])
        with api.Context(w, h, 1, 3, api.MODE_O if (w + h) % 2 else api.MODE_R) as ctx:   # either mode
            _varied(ctx, maps, "sizes")


CONTENTS = ("empty", "full", "nw", "ne", "sw", "se", "centre", "row", "column", "ends", "top-bottom", "345", "checkerboard", "sparse", "mixed")


@pytest.mark.parametrize("kind", CONTENTS)
def test_contents(kind):
    for w, h in ((2 * ROW_THREADS + 1, LOOKAHEAD + 1), (65, 21), (5, 1)):
        maps = np.stack([_content(kind, w, h, 7), _content("random0.1", w, h, 8)])   # a second frame of other content
        with api.Context(w, h, 1, 2) as ctx:
            for target in (NZ, ZERO):
                for dist_type in (SQ, F32):
                    d2, near = _call(ctx, maps, target, dist_type, True, w + 1, base_off=1, pad=(4, 8), what=kind)
                _call(ctx, maps, target, SQ, False, what=kind + " without nearest")
                if kind in ("empty", "full"):   # (the restatement's own answer: a frame without a feature pixel, or of nothing else)
                    none = (kind == "empty") == (target == NZ)
                    assert (d2[0] == (R.NONE if none else 0)).all() and (near[0] == -1).all() == none
    if kind == "ends":   # the tie of the issue: features at x = 0 and x = 4, the query x = 2 goes to x' = 0
        m = np.zeros((1, 3, 5), np.uint8)
        m[0, :, 0] = m[0, :, 4] = 255
        with api.Context(5, 3, 1, 1) as ctx:
            d2, near = _call(ctx, m, NZ, SQ, what="x = 0 and x = 4")
            assert d2[0, 1].tolist() == [0, 1, 4, 1, 0] and near[0, 1].tolist() == [5, 5, 5, 9, 9]


def test_frames_of_a_batch_are_independent():
    w, h = 2 * COL_THREADS + 1, 11
    kinds = ("sparse", "empty", "random0.5", "full", "centre", "checkerboard", "se")
    maps = np.stack([_content(k, w, h, 3) for k in kinds])
    with api.Context(w, h, 1, len(kinds)) as ctx:
        _call(ctx, maps, NZ, F32, True, w + 5, (w + 5) * h + 77, base_off=3, pad=(20, 4), gap=(4 * 333, 12), what="seven contents")
        _call(ctx, maps, ZERO, SQ, True, what="seven contents")
        for f in (0, 1, 4, 6):   # each frame alone gives the same planes
            _call(ctx, maps[f:f + 1], NZ, F32, what=f"frame {f} alone")


def test_the_widest_context():
    """8184 x 2, the widest frame hc_create takes: 32 strides of the 256 threads over a row, 32 KiB of LDS.  (The limit of the LDS
    row itself, 16384 columns, cannot be reached through a context: tests/test_dist_plan_cpu.py holds it.)  A feature pixel in the
    last column and one in the first of the other row, so that the search of the pixels in the middle runs over half the row on
    both sides; a sparse frame; an empty one."""
    w, h = 8184, 2
    a = np.zeros((h, w), np.uint8)
    a[0, w - 1] = a[1, 0] = 255
    maps = np.stack([a, _content("sparse", w, h, 1)])
    with api.Context(w, h, 1, 2) as ctx:
        d2, near = _call(ctx, maps, NZ, SQ, what="the widest")
        assert near[0, 0, 0] == w and near[0, 1, w - 1] == w - 1 and d2[0].max() > 4000 ** 2
        _call(ctx, maps, NZ, F32, True, w + 3, base_off=1, pad=(4, 0), what="the widest")
        _call(ctx, np.zeros((1, h, w), np.uint8), NZ, F32, what="the widest, empty")


def test_roots_above_2_to_the_24():
    """4100 x 2 with one feature pixel at (0, 0): d2 reaches 4099^2 + 1 > 2^24, where the conversion to float32 rounds.  In that
    frame the rule sqrtf((float)d2) and a root taken in double and rounded still give the same floats (d2 = x^2 or x^2 + 1); in
    8184 x 3 they differ in a thousand pixels of the third row, from d2 = 6145^2 + 2^2 = 37,761,029 on, so a kernel that took the
    other route would be seen there."""
    for w, h in ((4100, 2), (8184, 3)):
        m = np.zeros((1, h, w), np.uint8)
        m[0, 0, 0] = 1
        with api.Context(w, h, 1, 1) as ctx:
            d2, near = _call(ctx, m, NZ, F32, what="one pixel")
            assert d2.max() == (w - 1) ** 2 + (h - 1) ** 2 > 1 << 24 and (near == 0).all()
            differ = R.root_f32(d2) != np.sqrt(d2.astype(np.float64)).astype(np.float32)
            assert differ.any() == (h == 3) and (h == 2 or differ[0, 2, 6145])
            _call(ctx, m, NZ, SQ, False, what="one pixel")


def _bytes(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape[0], a.shape[1], -1)


def test_both_planes_as_rois_of_one_plane():
    """d_dist and d_nearest side by side in the rows of one plane (equal pitch and stride, touching, and with a gap), and one behind
    the other, the second beginning where the first ends: every byte of the plane outside the two views keeps its value."""
    import torch
    w, h, n = 65, 9, 3
    maps = np.stack([_content(k, w, h, 4) for k in ("random0.1", "mixed", "nw")])
    d2, near = _ref(maps, NZ)
    src = torch.from_numpy(maps).cuda()
    with api.Context(w, h, 1, n) as ctx:
        for dist_type, dist in ((SQ, d2), (F32, R.root_f32(d2))):
            for between in (0, 12):   # touching; three words of the caller's between the views
                row = 8 * w + between
                arena, g = VA.make_output(n, h, row, row + 20, (row + 20) * h + 40, 8, lead=VA.round_up(row + 84, 4), seed=between)
                d = torch.from_numpy(arena).cuda()
                torch.cuda.synchronize()
                base = d.data_ptr() + g.offset
                ctx.distance_transform_device(src.data_ptr(), w, w * h, n, NZ, dist_type, base, g.pitch, g.frame_stride, base + 4 * w + between, g.pitch, g.frame_stride)
                ctx.sync()
                before = VA.read_view(arena, g)
                want = np.concatenate((_bytes(dist), before[:, :, 4 * w:4 * w + between], _bytes(near)), axis=2)
                VA.check_output(d.cpu().numpy(), arena, g, want, what=f"side by side, {between} bytes between, type {dist_type}")
            # one behind the other: 2 n tight frames of one arena
            arena, g = VA.make_output(2 * n, h, 4 * w, 4 * w, None, 4, seed=9)
            d = torch.from_numpy(arena).cuda()
            torch.cuda.synchronize()
            base = d.data_ptr() + g.offset
            ctx.distance_transform_device(src.data_ptr(), w, w * h, n, NZ, dist_type, base, 4 * w, 4 * w * h, base + n * 4 * w * h, 4 * w, 4 * w * h)
            ctx.sync()
            VA.check_output(d.cpu().numpy(), arena, g, np.concatenate((_bytes(dist), _bytes(near))), what=f"touching, type {dist_type}")


def _scene(w, h, n, seed):
    return np.stack([synth.natural(w, h, seed + i) for i in range(n)])


def test_canny_distance_and_a_thresh_map():
    w, h, n = 160, 120, 2
    frames = _scene(w, h, n, 40)
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        edges = ctx.canny(frames, 50, 150)
        assert edges.any()
        d2, near = _ref(edges, NZ)
        got = ctx.canny_distance(frames, 50, 150)
        assert len(got) == 2 and np.array_equal(got[0], edges) and got[1].dtype == np.float32
        assert np.array_equal(got[1].view(np.uint32), R.root_f32(d2).view(np.uint32))
        got = ctx.canny_distance(frames, 50, 150, squared=True, nearest=True)
        assert np.array_equal(got[0], edges) and np.array_equal(got[1], d2) and np.array_equal(got[2], near) and got[1].dtype == got[2].dtype == np.int32
        blurred = ctx.blur_canny(frames, 5, 1.2, 50, 150)
        got = ctx.canny_distance(frames, 50, 150, blur=(5, 1.2), squared=True)
        assert np.array_equal(got[0], blurred) and np.array_equal(got[1], _ref(blurred, NZ)[0])
        _call(ctx, edges, NZ, F32, True, w + 1, base_off=1, what="canny maps")
        # the host wrapper: one map, the defaults; a torch tensor; cv::distanceTransform's own convention
        one = ctx.distance_transform(edges[0])
        assert one.shape == (1, h, w) and np.array_equal(one.view(np.uint32), R.root_f32(d2[:1]).view(np.uint32))
        import torch
        inv = ctx.distance_transform(torch.from_numpy(255 - edges).cuda(), api.DT_TO_ZERO, squared=True, nearest=True)
        assert np.array_equal(inv[0], d2) and np.array_equal(inv[1], near)
    with api.Context(w, h, 1, n, api.MODE_R) as ctx:   # the 0 / 128 / 255 of an HC_STAGE_THRESH map: both values are features
        ctx.upload(frames)
        ctx.run(api.CannyStage.THRESH, n)
        thr = ctx.download(n)
        assert {128, 255} <= set(np.unique(thr).tolist())
        _call(ctx, thr, NZ, SQ, what="THRESH map")


def test_behind_pipelined_runs_without_a_sync():
    """Pipelined runs into a ring of buffers as hc_pipeline_depth sizes it, then the transforms of every buffer with no
    synchronisation in between: the entry completes the runs that still write the maps it reads."""
    import torch
    w, h, n = 160, 96, 2
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        ctx.set_thresholds(40, 90)
        ctx.set_option(api.OPT_PIPELINE, 1)
        ring = ctx.pipeline_depth(n) + 1
        srcs = [torch.from_numpy(_scene(w, h, n, 70 + 10 * i)).cuda() for i in range(ring)]
        outs = [torch.zeros_like(s) for s in srcs]
        dist = [torch.full((n, h, w), -7, dtype=torch.int32, device="cuda") for _ in srcs]
        near = [torch.full((n, h, w), -7, dtype=torch.int32, device="cuda") for _ in srcs]
        torch.cuda.synchronize()
        for s, o in zip(srcs, outs):
            ctx.run_device(s.data_ptr(), w, w * h, o.data_ptr(), w, w * h, n)
        for k, o in enumerate(outs):
            ctx.distance_transform_device(o.data_ptr(), w, w * h, n, NZ, SQ if k % 2 else F32, dist[k].data_ptr(), 4 * w, 4 * w * h, near[k].data_ptr(), 4 * w, 4 * w * h)
        ctx.sync()
        for k, o in enumerate(outs):
            edges = o.cpu().numpy()
            assert edges.any()
            d2, nr = _ref(edges, NZ)
            want = d2 if k % 2 else R.root_f32(d2).view(np.int32)
            assert np.array_equal(dist[k].cpu().numpy(), want) and np.array_equal(near[k].cpu().numpy(), nr), f"buffer {k} of {ring}"


def test_not_a_run():
    w, h, n = 160, 120, 2
    frames = _scene(w, h, n, 40)   # (the maps of test_canny_distance_and_a_thresh_map: one restatement for both)
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        maps = ctx.canny(frames, 50, 150)
        def state():
            return ctx.hysteresis_schedule(), ctx.last_run_info(), ctx.pipeline_slots_in_use(), ctx.hysteresis_totals(), ctx.hysteresis_info()
        before = state()
        assert before[0]["launches"] > 0
        _call(ctx, maps, NZ, F32, what="after a run")
        _call(ctx, maps, ZERO, SQ, False, what="after a run")
        assert state() == before


def test_one_channel_maps_on_three_channel_contexts():
    """Edge maps have one channel on every context; with HC_OPT_PER_CHANNEL the frame limit is 3 * max_batch."""
    w, h, mb = 37, 21, 2
    maps = np.stack([_content(("random0.1", "sparse", "mixed", "centre", "row", "empty", "full")[k], w, h, k) for k in range(3 * mb + 1)])
    with api.Context(w, h, 3, mb, api.MODE_O) as ctx:
        _call(ctx, maps[:mb], NZ, F32, what="a 3-channel context")
        with pytest.raises(api.HipCannyError, match="hc_distance_transform_device: nframes out of range"):
            ctx.distance_transform(maps[:mb + 1])
        ctx.set_option(api.OPT_PER_CHANNEL, 1)
        _call(ctx, maps[:3 * mb], NZ, SQ, True, w + 3, base_off=2, pad=(4, 4), what="3 * max_batch maps")
        got = ctx.distance_transform(maps[:3 * mb], squared=True, nearest=True)
        assert np.array_equal(got[0], _ref(maps[:3 * mb], NZ)[0]) and np.array_equal(got[1], _ref(maps[:3 * mb], NZ)[1])
        with pytest.raises(api.HipCannyError, match="hc_distance_transform_device: nframes out of range"):
            ctx.distance_transform(maps)


def test_refusals():
    """Every refusal through the C ABI, by the entry's prefix; nothing is written."""
    import torch
    w, h = 16, 8
    CANARY = -0x5A5A5A5B
    d = torch.full((2, h, w), 255, dtype=torch.uint8, device="cuda")
    dist = torch.full((2 * h * w + 8,), CANARY, dtype=torch.int32, device="cuda")
    near = torch.full((2 * h * w + 8,), CANARY, dtype=torch.int32, device="cuda")
    both = torch.full((9 * h * w + 64,), 255, dtype=torch.uint8, device="cuda")   # a map with its planes right behind it
    m, l, q, u = d.data_ptr(), dist.data_ptr(), near.data_ptr(), both.data_ptr()
    assert l % 4 == 0 and q % 4 == 0 and u % 4 == 0
    torch.cuda.synchronize()
    fs, lp, lfs = w * h, 4 * w, 4 * w * h
    big = 1 << 64
    with api.Context(w, h, 1, 2) as ctx:
        good = (m, w, fs, 1, NZ, F32, l, lp, lfs, q, lp, lfs)
        two = good[:3] + (2,) + good[4:]
        bad = {
            "d_map null": ("null argument", (0,) + good[1:]),
            "d_dist null": ("null argument", good[:6] + (0,) + good[7:]),
            "target 2": ("target must be", good[:4] + (2,) + good[5:]),
            "target -1": ("target must be", good[:4] + (-1,) + good[5:]),
            "dist_type 2": ("dist_type must be", good[:5] + (2,) + good[6:]),
            "dist_type -1": ("dist_type must be", good[:5] + (-1,) + good[6:]),
            "pitch < W": ("pitch smaller than a row", (m, w - 1) + good[2:]),
            "d_dist misaligned": ("multiples of", good[:6] + (l + 2,) + good[7:]),
            "dist_pitch no multiple of 4": ("multiples of", good[:7] + (lp + 2,) + good[8:]),
            "dist_frame_stride no multiple of 4": ("multiples of", two[:8] + (lfs + 2,) + two[9:]),
            "d_nearest misaligned": ("multiples of", good[:9] + (q + 1, lp, lfs)),
            "nearest_pitch no multiple of 4": ("multiples of", good[:9] + (q, lp + 2, lfs)),
            "nearest_frame_stride no multiple of 4": ("multiples of", two[:9] + (q, lp, lfs + 2)),
            "dist_pitch < 4 W": ("pitch smaller than a row", good[:7] + (lp - 4,) + good[8:]),
            "nearest_pitch < 4 W": ("pitch smaller than a row", good[:9] + (q, lp - 4, lfs)),
            "H * pitch >= 2^32": ("4 GiB", (m, 1 << 29, 1 << 32) + good[3:]),
            "H * dist_pitch >= 2^32": ("4 GiB", good[:7] + (1 << 29, 1 << 32) + good[9:]),
            "H * nearest_pitch >= 2^32": ("4 GiB", good[:9] + (q, 1 << 29, 1 << 32)),
            "nframes 0": ("nframes out of range", good[:3] + (0,) + good[4:]),
            "nframes -1": ("nframes out of range", good[:3] + (-1,) + good[4:]),
            "nframes 3 of 2": ("nframes out of range", good[:3] + (3,) + good[4:]),
            "map frame stride below a frame": ("frame stride below height * pitch", (m, w, fs - 1) + two[3:]),
            "dist frame stride below a frame": ("frame stride below height * pitch", two[:8] + (lfs - 4,) + two[9:]),
            "nearest frame stride below a frame": ("frame stride below height * pitch", two[:9] + (q, lp, lfs - 4)),
            "a map that wraps the address space": ("wraps the address space", (big - 64,) + good[1:]),
            "distances that wrap the address space": ("wraps the address space", good[:6] + (big - 64,) + good[7:]),
            "nearest that wraps the address space": ("wraps the address space", good[:9] + (big - 64, lp, lfs)),
            "distances inside the map": ("the map and the distance plane overlap", (u, w, fs, 1, NZ, SQ, u + fs - 4, lp, lfs, u + 5 * fs, lp, lfs)),
            "the map inside the distances": ("the map and the distance plane overlap", (u + 4, w, fs, 1, NZ, SQ, u, lp, lfs, u + 5 * fs, lp, lfs)),
            "nearest inside the map": ("the map and the nearest plane overlap", (u, w, fs, 1, NZ, SQ, u + 5 * fs, lp, lfs, u + fs - 4, lp, lfs)),
            "nearest inside the distances": ("the distance plane and the nearest plane overlap", (u, w, fs, 1, NZ, SQ, u + fs, lp, lfs, u + 5 * fs - 4, lp, lfs)),
            "one plane for both": ("the distance plane and the nearest plane overlap", good[:9] + (l, lp, lfs)),
        }
        for name, (text, args) in bad.items():
            with pytest.raises(api.HipCannyError, match="error -1"):
                ctx.distance_transform_device(*args)
            assert "hc_distance_transform_device: " in api.last_error() and text in api.last_error(), (name, api.last_error())
        assert api.load_library().hc_distance_transform_device(None, *good) == -1   # ctx null
        assert "hc_distance_transform_device: null argument" in api.last_error()
        ctx.sync()
        torch.cuda.synchronize()
        assert (dist.cpu().numpy() == CANARY).all() and (near.cpu().numpy() == CANARY).all() and (both.cpu().numpy() == 255).all() and (d.cpu().numpy() == 255).all()
        # views that merely touch are fine: the distances begin where the map ends, the nearest plane where they end
        ctx.distance_transform_device(u, w, fs, 1, NZ, SQ, u + fs, lp, lfs, u + 5 * fs, lp, lfs)
        ctx.distance_transform_device(m, w, fs, 2, ZERO, SQ, l, lp, lfs, None, 3, 1)   # no nearest plane: its pitch and stride are not looked at
        ctx.sync()
        b = both.cpu().numpy()
        assert (b[:fs] == 255).all() and (b[fs:5 * fs] == 0).all() and np.array_equal(b[5 * fs:9 * fs].view(np.int32), np.arange(fs)) and (b[9 * fs:] == 255).all()
        assert (dist.cpu().numpy()[:2 * h * w] == R.NONE).all() and (dist.cpu().numpy()[2 * h * w:] == CANARY).all() and (near.cpu().numpy() == CANARY).all()
    # (W * H >= 2^31 - 1 and W > 16384 cannot be reached here: hc_create takes no context wider than 8184 columns.
    # tests/test_dist_plan_cpu.py holds those two refusals.)  The squared diagonal, on a frame of two columns:
    tall = 46342
    with api.Context(2, tall, 1, 1) as ctx:
        col = torch.zeros((tall, 2), dtype=torch.uint8, device="cuda")
        out = torch.full((tall, 2), CANARY, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(api.HipCannyError, match="error -1"):
            ctx.distance_transform_device(col.data_ptr(), 2, 2 * tall, 1, NZ, SQ, out.data_ptr(), 8, 8 * tall)
        assert "hc_distance_transform_device: the squared diagonal" in api.last_error()
        ctx.sync()
        assert (out.cpu().numpy() == CANARY).all()


@pytest.mark.parametrize("seed", [20261021, 20261022, 20261023, 20261024])
def test_fuzz(seed):
    """Seeded: random shapes up to 300 x 40, densities, targets, types and view geometries."""
    rng = np.random.default_rng(seed)
    for it in range(10):
        w, h, n = int(rng.integers(1, 301)), int(rng.integers(1, 41)), int(rng.integers(1, 4))
        density = float(rng.choice([0.0, 0.002, 0.02, 0.1, 0.5, 0.97, 1.0]))
        maps = np.where(rng.random((n, h, w)) < density, rng.integers(1, 256, (n, h, w)), 0).astype(np.uint8)
        mp = w + int(rng.integers(0, 9))
        with api.Context(w, h, 1, n) as ctx:
            _call(ctx, maps, int(rng.integers(0, 2)), int(rng.integers(0, 2)), bool(rng.integers(0, 4)), mp, mp * h + int(rng.integers(0, 20)), base_off=int(rng.integers(0, 4)),
                  pad=(4 * int(rng.integers(0, 5)), 4 * int(rng.integers(0, 5))), gap=(4 * int(rng.integers(0, 9)), 4 * int(rng.integers(0, 9))),
                  off=(4 * int(rng.integers(0, 4)), 4 * int(rng.integers(0, 4))), fill=("ff", "random")[it % 2], what=f"fuzz {it} density {density}")
