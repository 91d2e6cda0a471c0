"""hc_thinning_device (k_thin_pack, k_thin_step, k_thin_unpack) on the MI355X: Zhang-Suen and Guo-Hall thinning through the C ABI,
byte for byte against tests/thin_ref.py (anchored by tests/test_thin_ref_cpu.py).  Every call goes through _call: the map, the
output and the status table are views of guarded arenas, and every byte of every arena is compared -- the output view and the
status words with the reference, everything else with what it held before.
Shapes around the dword, panel (64 words = 2048 columns) and tile (THIN_TILE_ROWS rows) seams; empty, full, blob, noise, bar,
band and seam-block contents and closed cv::Canny maps; the per-frame stop; cut and continue; caller views; passes under a small
scratch bound; the refusals; the chains behind cv::Canny and a closing and ahead of the components and point lists, also behind
pipelined runs and across a stream switch; the Python layer; repeatability."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cudacam_amd import api, synth
import ccl_ref
import edge_points_ref
import morph_ref as M
import thin_ref as T
import view_arena as VA

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _param(name):
    src = open(os.path.join(ROOT, "cudacam_amd", "csrc", "canny_params.h")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


TILE = _param("THIN_TILE_ROWS")
PANEL_PX = 32 * _param("THIN_PANEL_WORDS")
assert PANEL_PX == 2048   # (the widths below name the wave's 2048 columns +- 1)
STATUS_GUARD = 0xA5A5A5A5


# ---- content ---------------------------------------------------------------------------------------------------------------------
def _seam_blocks(h, w, size):
    """size + 1 frames of isolated size x size blocks, one block at every (column seam, row seam) pair.  The column seams are the
    dword seams (every 32 columns, so the panel seams at every 2048 too), the row seams the tile seams; a shape without one
    takes its middle column / row instead.  In frame k every block begins size - k columns left of its column seam: k = 0 lies
    left of the seam and ends on its last column, k = 1 .. size - 1 straddle it by every amount, k = size begins on it.  Rows
    likewise: size - k rows above the tile seam at even column seams, k rows above it at odd ones, so that over the frames every
    tile seam also sees every offset at either parity.  Seams are 32 columns / TILE rows apart and a block reaches at most `size`
    beyond one, so the blocks stay isolated."""
    cols = list(range(32, w, 32)) or [w // 2]
    rows = list(range(TILE, h, TILE)) or [h // 2]
    frames = []
    for k in range(size + 1):
        m = np.zeros((h, w), np.uint8)
        for i, c in enumerate(cols):
            for r in rows:
                x = c - size + k
                y = r - size + (k if i % 2 == 0 else size - k)
                m[max(y, 0):max(y + size, 0), max(x, 0):max(x + size, 0)] = 255
        frames.append(m)
    return frames


def _contents(h, w, seed):
    """[empty, full, blobs, noise at 0.5, bars four rows thick, diagonal bands, the 3 frames of 2 x 2 seam blocks, the 4 frames of
    3 x 3 seam blocks]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([
        np.zeros((h, w), np.uint8),
        np.full((h, w), 255, np.uint8),
        T.blobs(h, w, seed),
        ((rng.random((h, w)) < 0.5) * rng.integers(1, 256, (h, w))).astype(np.uint8),   # (foreground: any non-zero byte)
        ((yy % 9 < 4) * 255).astype(np.uint8),
        (((xx + yy) % 13 < 5) * 255).astype(np.uint8),
    ] + _seam_blocks(h, w, 2) + _seam_blocks(h, w, 3))


def test_seam_blocks_lie_on_both_sides_of_every_seam_and_straddle_it():
    """The content itself, on the shapes with a panel seam and with tile seams: at every column seam and every tile seam, over the
    frames of a size, a block that ends on the seam's last column / row, blocks that straddle it by every amount, and one that
    begins on it; inside the frame every block is whole and isolated."""
    from scipy import ndimage
    for h, w in ((9, PANEL_PX + 1), (3, 2080), (2 * TILE + 1, 70)):
        for size in (2, 3):
            frames = _seam_blocks(h, w, size)
            assert len(frames) == size + 1
            for c in range(32, w, 32):
                starts = set()
                for m in frames:
                    xs = np.flatnonzero(m[:, max(c - size, 0):c + size].any(axis=0)) + max(c - size, 0)
                    starts.add(int(xs.min()) - c)
                    assert xs.max() - xs.min() + 1 == min(size, w - xs.min())
                assert starts == set(range(-size, 1)), (h, w, size, c, starts)
            for r in range(TILE, h, TILE):
                for parity in (0, 1):
                    cs = [c for i, c in enumerate(range(32, w, 32)) if i % 2 == parity]
                    starts = {int(np.flatnonzero(m[max(r - size, 0):r + size, cs[0] - size:cs[0] + size].any(axis=1)).min()) + max(r - size, 0) - r for m in frames}
                    assert starts == set(range(-size, 1)), (h, w, size, r, parity, starts)
            if h >= size and w > 32 + size:
                for m in frames:
                    lab, n = ndimage.label(m, structure=np.ones((3, 3), int))
                    assert n == len(range(32, w, 32)) * max(len(range(TILE, h, TILE)), 1)
                    assert (ndimage.sum(m > 0, lab, range(1, n + 1)) <= size * size).all()


def _scene(w, h, n, seed):
    return np.stack([synth.natural(w, h, seed + i) for i in range(n)])


def _closed_canny(w, h, seed):
    """cv::Canny maps of two synthetic frames, closed with 3 x 3 RECT and with 5 x 5 ELLIPSE (by the entries that have their own
    tests): [2 x 2, H, W]"""
    frames = _scene(w, h, 2, seed)
    with api.Context(w, h, 1, 2, api.MODE_O) as ctx:
        edges = ctx.canny(frames, 60, 150)
        return np.concatenate([ctx.morphology(edges, api.MORPH_CLOSE, api.MORPH_RECT, 3), ctx.morphology(edges, api.MORPH_CLOSE, api.MORPH_ELLIPSE, 5)])


# ---- one call on guarded arenas --------------------------------------------------------------------------------------------------
def _lead(pitch):
    return VA.round_up(pitch + 64, 16)   # the view's alignment is that of its base offset


def _call(ctx, maps, method, max_it, want=None, in_pitch=None, in_fs=None, in_off=0, pitch=None, fs=None, out_off=0, status=True, seed=0, what=""):
    """Thins `maps` [n, H, W] and checks everything; returns (maps, status) as the device wrote them.  want: (maps, status) instead
    of the reference's."""
    import torch
    n, h, w = maps.shape
    in_pitch = w if in_pitch is None else in_pitch
    pitch = w if pitch is None else pitch
    a_in, off_in = VA.make_input(maps, in_pitch, in_fs, in_off, "random", lead=_lead(in_pitch), seed=seed)
    b_out, g_out = VA.make_output(n, h, w, pitch, fs, out_off, lead=_lead(pitch), seed=seed + 1)
    st0 = np.full(2 * n + 8, STATUS_GUARD, np.uint32)
    d_in, d_out, d_st = (torch.from_numpy(v).cuda() for v in (a_in, b_out, st0.view(np.int32)))
    torch.cuda.synchronize()
    ctx.thinning_device(d_in.data_ptr() + off_in, in_pitch, in_pitch * h if in_fs is None else in_fs, d_out.data_ptr() + g_out.offset, pitch, g_out.frame_stride, n, method, max_it,
                        d_st.data_ptr() + 16 if status else None)
    ctx.sync()
    ref_maps, ref_st = T.thin_batch(maps, method, max_it) if want is None else want
    what = f"{what} method {method} max_iterations {max_it} {w}x{h}x{n} in(pitch {in_pitch}, off {in_off}) out(pitch {pitch}, off {out_off})"
    after = d_out.cpu().numpy()
    VA.check_output(after, b_out, g_out, ref_maps, what)
    assert np.array_equal(d_in.cpu().numpy(), a_in), "the map's arena was written: " + what
    st = d_st.cpu().numpy().view(np.uint32)
    want_st = st0.copy()
    if status:
        want_st[4:4 + 2 * n] = np.asarray(ref_st, np.uint32).reshape(-1)
    assert np.array_equal(st, want_st), f"status {st[4:4 + 2 * n].reshape(n, 2).tolist()} want {np.asarray(ref_st).tolist()} (guards {st[:4].tolist()} {st[4 + 2 * n:].tolist()}): {what}"
    return VA.read_view(after, g_out).reshape(n, h, w), st[4:4 + 2 * n].reshape(n, 2).copy()


# ---- shapes and content ----------------------------------------------------------------------------------------------------------
WIDTHS = [1, 2, 31, 32, 33, 63, 64, 65, PANEL_PX - 1, PANEL_PX, PANEL_PX + 1, 2080]
SHAPES = [(w, h) for w in WIDTHS for h in (1, 2, 3, 9)] + [(70, h) for h in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1)]


@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_shapes_and_contents(w, h):
    maps = _contents(h, w, 100 * w + h)
    with api.Context(w, h, 1, len(maps), api.MODE_O) as ctx:
        for method in T.METHODS:
            _, st = _call(ctx, maps, method, 24, seed=w + h)
            assert (st[:, 1] == 1).all(), "24 iterations reach the fixed point of frames at most 33 rows thick"


def test_closed_canny_maps():
    w, h = 640, 360
    maps = _closed_canny(w, h, 11)
    assert maps.any(axis=(1, 2)).all()
    with api.Context(w, h, 1, len(maps), api.MODE_O) as ctx:
        for method in T.METHODS:
            got, st = _call(ctx, maps, method, 16)
            assert (st[:, 1] == 1).all() and (st[:, 0] >= 1).all() and (got.astype(bool).sum(axis=(1, 2)) < maps.astype(bool).sum(axis=(1, 2))).all()


def test_1080p():
    """68 tiles of 60 lanes: a closed cv::Canny map and blobs, one method each (the reference takes a second per frame here)."""
    w, h = 1920, 1080
    maps = np.stack([_closed_canny(w, h, 3)[2], T.blobs(h, w, 5)])
    with api.Context(w, h, 1, 2, api.MODE_O) as ctx:
        _call(ctx, maps[:1], T.GUOHALL, 16)
        _call(ctx, maps[1:], T.ZHANGSUEN, 16)


# ---- per-frame stop, cut and continue ----------------------------------------------------------------------------------------
def _thick(h, w, rows):
    m = np.zeros((h, w), np.uint8)
    m[6:6 + rows, 5:w - 7] = 255
    return m


def test_per_frame_stop():
    h, w = 100, 150
    line = np.zeros((h, w), np.uint8)   # a thin line: two pixels thick, so that it takes one iteration and the empty frame none
    line[50:52, 10:140] = 255
    maps = np.stack([np.zeros((h, w), np.uint8), line, _thick(h, w, 40), T.blobs(h, w, 9)])
    with api.Context(w, h, 1, 4, api.MODE_O) as ctx:
        for method in T.METHODS:
            ref = T.thin_batch(maps, method, 32)
            assert ref[1][0].tolist() == [0, 1] and (ref[1][:, 1] == 1).all()
            assert len(set(ref[1][:, 0].tolist())) == 4 and ref[1][2, 0] >= 15, "the iteration counts of the four frames all differ"
            _call(ctx, maps, method, 32, want=ref)
            _call(ctx, maps[::-1].copy(), method, 32)   # the order of the frames does not matter
            _call(ctx, maps, method, 32, want=ref, status=False)


def test_cut_and_continue():
    h, w = 60, 90
    m = _thick(h, w, 40)[None]
    with api.Context(w, h, 1, 1, api.MODE_O) as ctx:
        for method in T.METHODS:
            full, total, conv = T.thin(m[0], method, 64)
            assert conv == 1 and total > 6
            for n1 in (1, 2, 3):
                part, st = _call(ctx, m, method, n1)
                assert st.tolist() == [[n1, 0]]
                rest, st2 = _call(ctx, part, method, 64)
                assert np.array_equal(rest[0], full) and st2.tolist() == [[total - n1, 1]]
                exact, st3 = _call(ctx, part, method, total - n1)   # the remaining count alone: the fixed point, not yet known as one
                assert np.array_equal(exact[0], full) and st3.tolist() == [[total - n1, 0]]


def test_max_iterations_1_and_1024():
    h, w = 5, 40
    maps = _contents(h, w, 3)[[1, 5]]
    with api.Context(w, h, 1, 2, api.MODE_R) as ctx:   # (contexts of either mode)
        _call(ctx, maps, T.ZHANGSUEN, 1)
        _, st = _call(ctx, maps, T.GUOHALL, 1024)
        assert (st[:, 1] == 1).all()


# ---- views -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(70, 2 * TILE + 1), (PANEL_PX + 5, 3), (1, 4)])
def test_views(w, h):
    """Both views as ROIs of larger planes: base offsets 0..3, tight, odd and padded pitches, a frame stride with a gap, 4-aligned
    views (dword loads / stores) and others, poisoned guards all around."""
    maps = _contents(h, w, 7 + w)[[2, 3, 7, 10]]   # blobs, noise, blocks that straddle the seams: 2 x 2 by one column, 3 x 3 by one
    with api.Context(w, h, 1, len(maps), api.MODE_O) as ctx:
        ref = {m: T.thin_batch(maps, m, 20) for m in T.METHODS}
        c = 0
        for in_off in range(4):
            for out_off in range(4):
                in_al = 4 if in_off == 0 and c % 2 == 0 else 1
                out_al = 4 if out_off == 0 and c % 4 < 2 else 1
                in_pitch = VA.round_up(w + (0, 3, 4, 13)[c % 4], in_al)
                in_fs = VA.round_up(in_pitch * h + 5 * (c % 3), in_al)
                pitch = VA.round_up(w + (0, 5, 8, 1)[(c // 2) % 4], out_al)
                fs = VA.round_up(pitch * h + 3 * (c % 4), out_al)
                _call(ctx, maps, c % 2, 20, want=ref[c % 2], in_pitch=in_pitch, in_fs=in_fs, in_off=in_off, pitch=pitch, fs=fs, out_off=out_off, seed=c)
                c += 1


def test_touching_and_overlapping_views():
    import torch
    w, h, n = 45, 19, 2
    maps = _contents(h, w, 5)[[2, 5]]
    fs = w * h
    want, want_st = T.thin_batch(maps, T.GUOHALL, 20)
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        for order in (0, 1):   # the output directly behind / directly before the map
            host = np.full(2 * n * fs + 64, 77, np.uint8)
            i0, o0 = (32, 32 + n * fs) if order == 0 else (32 + n * fs, 32)
            host[i0:i0 + n * fs] = maps.reshape(-1)
            both = torch.from_numpy(host).cuda()
            torch.cuda.synchronize()
            ctx.thinning_device(both.data_ptr() + i0, w, fs, both.data_ptr() + o0, w, fs, n, T.GUOHALL, 20)
            ctx.sync()
            after = both.cpu().numpy()
            expect = host.copy()
            expect[o0:o0 + n * fs] = want.reshape(-1)
            assert np.array_equal(after, expect), f"touching views, order {order}"
            for shift in (1, n * fs - 1, fs):   # one shared byte on either side, a shared frame
                for d_out in (both.data_ptr() + i0 + n * fs - shift, both.data_ptr() + i0 - n * fs + shift):
                    with pytest.raises(api.HipCannyError, match="hc_thinning_device: the map and the output view overlap"):
                        ctx.thinning_device(both.data_ptr() + i0, w, fs, d_out, w, fs, n, T.GUOHALL, 20)
            with pytest.raises(api.HipCannyError, match="overlap"):
                ctx.thinning_device(both.data_ptr() + i0, w, fs, both.data_ptr() + i0, w, fs, n, T.GUOHALL, 20)
            ctx.sync()
            assert np.array_equal(both.cpu().numpy(), expect), "a refused call wrote"


# ---- passes ------------------------------------------------------------------------------------------------------------------------
def test_passes_under_a_small_scratch_bound():
    """A batch of 5 in 1, 3 and 5 passes gives the same bytes and status; a bound below one frame is refused."""
    w, h, mi = 131, 37, 24
    maps = _contents(h, w, 21)[[1, 2, 3, 5, 7]]
    frame = 2 * 4 * h * ((w + 31) // 32) + 4 * (mi + 1)
    want = T.thin_batch(maps, T.ZHANGSUEN, mi)
    assert len(set(want[1][:, 0].tolist())) > 2
    with api.Context(w, h, 1, 5, api.MODE_O) as ctx:
        for bound in (0, 2 * frame, 3 * frame - 1, frame, 2 * frame - 1, 5 * frame):   # 1, 3, 3, 5, 5, 1 passes; 0: the default
            ctx.set_option(api.OPT_TEST_HOUGH_SCRATCH, bound)
            _call(ctx, maps, T.ZHANGSUEN, mi, want=want, what=f"bound {bound}")
        ctx.set_option(api.OPT_TEST_HOUGH_SCRATCH, frame - 1)
        with pytest.raises(api.HipCannyError, match="hc_thinning_device: one frame of bit planes exceeds the context's scratch bound"):
            _call(ctx, maps, T.ZHANGSUEN, mi, want=want)
        ctx.set_option(api.OPT_TEST_HOUGH_SCRATCH, 0)
        _call(ctx, maps, T.GUOHALL, mi, what="after the refusal")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """Every refusal of the header through the C entry, with the entry's name in hc_last_error; nothing is written; the following
    valid call is still correct."""
    import torch
    w, h, n = 33, 12, 2
    maps = _contents(h, w, 6)[[2, 3]]
    fs = w * h
    with api.Context(w, h, 1, n, api.MODE_O) as ctx, api.Context(w, h, 3, n, api.MODE_O) as pc:
        pc.set_option(api.OPT_PER_CHANNEL, 1)
        src = torch.from_numpy(np.concatenate([maps] * 4)).cuda()   # 8 maps: beyond 3 * max_batch of the per-channel context
        guard = np.full((4 * n, h, w), 93, np.uint8)
        dst = torch.from_numpy(guard).cuda()
        st_guard = np.full(8 * n + 2, 0x5A5A5A5A, np.int32)
        st = torch.from_numpy(st_guard).cuda()
        torch.cuda.synchronize()
        L = ctx.lib

        def call(handle=ctx.handle, d_in=src.data_ptr(), ip=w, ifs=fs, d_out=dst.data_ptr(), op=w, ofs=fs, nf=n, method=0, mi=16, d_st=st.data_ptr()):
            return L.hc_thinning_device(handle, C.c_void_p(d_in), ip, ifs, C.c_void_p(d_out), op, ofs, nf, method, mi, C.c_void_p(d_st))
        bad = [
            ("null", dict(handle=None)), ("null", dict(d_in=None)), ("null", dict(d_out=None)),
            ("method must be", dict(method=2)), ("method must be", dict(method=-1)),
            ("max_iterations outside 1..1024", dict(mi=0)), ("max_iterations outside 1..1024", dict(mi=1025)), ("max_iterations outside 1..1024", dict(mi=-3)),
            ("d_status must be 4-byte aligned", dict(d_st=st.data_ptr() + 2)), ("d_status must be 4-byte aligned", dict(d_st=st.data_ptr() + 1)),
            ("pitch smaller than a row", dict(ip=w - 1)), ("pitch smaller than a row", dict(op=w - 1)),
            ("2^32", dict(ip=(1 << 32) // h + 1, ifs=((1 << 32) // h + 1) * h, nf=1)), ("2^32", dict(op=(1 << 32) // h + 1, ofs=((1 << 32) // h + 1) * h, nf=1)),
            ("nframes out of range", dict(nf=0)), ("nframes out of range", dict(nf=n + 1)), ("nframes out of range", dict(nf=-1)),
            ("nframes out of range", dict(handle=pc.handle, nf=3 * n + 1)),
            ("frame stride below", dict(ifs=fs - 1)), ("frame stride below", dict(ofs=fs - 1)),
            ("wraps the address space", dict(d_in=(1 << 64) - 100, nf=1)), ("wraps the address space", dict(d_out=(1 << 64) - 100, nf=1)),
            ("overlap", dict(d_out=src.data_ptr())), ("overlap", dict(d_out=src.data_ptr() + n * fs - 1)), ("overlap", dict(d_in=dst.data_ptr() + n * fs - 1)),
        ]
        for text, kw in bad:
            assert call(**kw) == -1, (text, kw)
            err = L.hc_last_error().decode()
            assert err.startswith("hc_thinning_device: ") and text in err, (text, err)
        ctx.sync()
        pc.sync()
        assert np.array_equal(dst.cpu().numpy(), guard) and np.array_equal(st.cpu().numpy(), st_guard), "a refused call wrote"
        # the neighbours that pass: a null status, the per-channel limit itself, max_iterations 1
        assert call(d_st=None, mi=1) == 0
        ctx.sync()
        assert np.array_equal(dst.cpu().numpy()[:n], T.thin_batch(maps, T.ZHANGSUEN, 1)[0]) and np.array_equal(st.cpu().numpy(), st_guard)
        assert call(handle=pc.handle, nf=3 * n) == 0
        pc.sync()
        want, want_st = T.thin_batch(np.concatenate([maps] * 3), T.ZHANGSUEN, 16)
        assert np.array_equal(dst.cpu().numpy()[:3 * n], want) and np.array_equal(dst.cpu().numpy()[3 * n:], guard[3 * n:])
        got_st = st.cpu().numpy()
        assert np.array_equal(got_st[:6 * n].view(np.uint32).reshape(-1, 2), want_st) and np.array_equal(got_st[6 * n:], st_guard[6 * n:])


# ---- chains ------------------------------------------------------------------------------------------------------------------------
def test_chain_canny_close_thin_components_and_points():
    """canny_device -> morphology (CLOSE) -> thinning -> connected_components and -> edge_points on one stream with no
    synchronisation in between, against the host model: the device's Canny map through morph_ref, thin_ref, ccl_ref and
    edge_points_ref."""
    import torch
    w, h, n = 320, 200, 3
    frames = _scene(w, h, n, 40)
    fs = w * h
    spans = M.structuring_spans(M.RECT, 3)
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        for method in T.METHODS:
            src = torch.from_numpy(frames).cuda()
            edges, closed, skel = (torch.full((n, h, w), 7, dtype=torch.uint8, device="cuda") for _ in range(3))
            labels = torch.empty((n, h, w), dtype=torch.int32, device="cuda")
            counts, pcounts = (torch.empty((n,), dtype=torch.int32, device="cuda") for _ in range(2))
            status = torch.empty((n, 2), dtype=torch.int32, device="cuda")
            cap = w * h
            pts = torch.empty((n, cap, 2), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ctx.canny_device(src.data_ptr(), w, fs, edges.data_ptr(), w, fs, n, 60, 150)
            ctx.morphology_device(edges.data_ptr(), w, fs, closed.data_ptr(), w, fs, n, 1, api.MORPH_CLOSE, 3, spans)
            ctx.thinning_device(closed.data_ptr(), w, fs, skel.data_ptr(), w, fs, n, method, 16, status.data_ptr())
            ctx.connected_components_device(skel.data_ptr(), w, fs, n, 8, labels.data_ptr(), 4 * w, 4 * fs, counts.data_ptr())
            ctx.edge_points_device(skel.data_ptr(), w, fs, n, pcounts.data_ptr(), pts.data_ptr(), cap)
            ctx.sync()
            assert ctx.hysteresis_info()[1] == 0, "the run was continued from the host: the maps changed behind the chain"
            e = edges.cpu().numpy()
            assert e.any()
            want, want_st = T.thin_batch(M.morph(e, M.CLOSE, spans), method, 16)
            assert np.array_equal(skel.cpu().numpy(), want) and np.array_equal(status.cpu().numpy().view(np.uint32), want_st)
            assert (want_st[:, 1] == 1).all()
            ref_labels, ref_counts, _, _ = ccl_ref.connected_components(want, 8)
            assert np.array_equal(labels.cpu().numpy(), ref_labels) and np.array_equal(counts.cpu().numpy().view(np.uint32), ref_counts)
            ref_pc, ref_pts = edge_points_ref.edge_points(want)
            assert np.array_equal(pcounts.cpu().numpy().view(np.uint32), ref_pc)
            got_pts = pts.cpu().numpy()
            for f in range(n):
                assert np.array_equal(got_pts[f, :int(ref_pc[f])], ref_pts[f])


def test_behind_pipelined_runs_and_not_a_run():
    """The entry reads the output of pipelined runs still in flight (it must complete them first), and it is not a run."""
    import torch
    w, h, n = 256, 128, 2
    sets = [_scene(w, h, n, 70 + 10 * i) for i in range(3)]
    fs = w * h
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        ctx.set_thresholds(40, 90)
        ctx.set_option(api.OPT_PIPELINE, 1)
        srcs = [torch.from_numpy(s).cuda() for s in sets]
        outs = [torch.empty_like(s) for s in srcs]
        dsts = [torch.empty_like(s) for s in srcs]
        torch.cuda.synchronize()
        for s, o in zip(srcs, outs):
            ctx.run_device(s.data_ptr(), w, fs, o.data_ptr(), w, fs, n)
        for i, (o, d) in enumerate(zip(outs, dsts)):
            ctx.thinning_device(o.data_ptr(), w, fs, d.data_ptr(), w, fs, n, i % 2, 8)
        ctx.sync()
        for i, (o, d) in enumerate(zip(outs, dsts)):
            edges = o.cpu().numpy()
            assert edges.any()
            assert np.array_equal(d.cpu().numpy(), T.thin_batch(edges, i % 2, 8)[0]), "behind a pipelined run"
        info = (C.c_int * len(api.SCHEDULE_FIELDS))()
        ri = [C.c_int(-5) for _ in range(3)]

        def state():
            assert ctx.lib.hc_last_hysteresis_schedule(ctx.handle, info, len(info)) >= 0
            assert ctx.lib.hc_last_run_info(ctx.handle, *[C.byref(v) for v in ri]) == 0
            return list(info), [v.value for v in ri], ctx.hysteresis_info()
        before = state()
        ctx.thinning_device(outs[0].data_ptr(), w, fs, dsts[1].data_ptr(), w, fs, n, T.GUOHALL, 8)
        ctx.sync()
        assert state() == before
        assert np.array_equal(dsts[1].cpu().numpy(), T.thin_batch(outs[0].cpu().numpy(), T.GUOHALL, 8)[0])


def test_stream_switch_between_two_calls_that_share_the_scratch():
    import torch
    w, h, n = 300, 90, 3
    a, b = _contents(h, w, 31)[[1, 2, 5]], _contents(h, w, 32)[[3, 2, 7]]
    fs = w * h
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        oa, ob = torch.empty_like(da), torch.empty_like(db)
        sa, sb = (torch.empty((n, 2), dtype=torch.int32, device="cuda") for _ in range(2))
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        ctx.thinning_device(da.data_ptr(), w, fs, oa.data_ptr(), w, fs, n, T.ZHANGSUEN, 48, sa.data_ptr())
        ctx.set_stream(s.cuda_stream)
        ctx.thinning_device(db.data_ptr(), w, fs, ob.data_ptr(), w, fs, n, T.GUOHALL, 48, sb.data_ptr())
        ctx.sync()
        ctx.use_own_stream()
        ctx.sync()
        torch.cuda.synchronize()
        for got, st, maps, method in ((oa, sa, a, T.ZHANGSUEN), (ob, sb, b, T.GUOHALL)):
            want, want_st = T.thin_batch(maps, method, 48)
            assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(st.cpu().numpy().view(np.uint32), want_st)


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
def test_context_thinning_in_chunks():
    """max_iterations=None on a 60-row-thick rectangle: several chunks of 16 iterations."""
    h, w = 80, 120
    maps = np.stack([_thick(h, w, 60), T.blobs(h, w, 2), np.zeros((h, w), np.uint8)])
    with api.Context(w, h, 1, 3, api.MODE_O) as ctx:
        for name, method in api.THIN_METHODS.items():
            want, want_st = T.thin_batch(maps, method, 200)
            assert want_st[0, 0] > 16 and (want_st[:, 1] == 1).all()
            got, it, conv = ctx.thinning(maps, method=name, max_iterations=None)
            assert np.array_equal(got, want) and it.tolist() == want_st[:, 0].tolist() and conv.tolist() == [1, 1, 1]
            got, it, conv = ctx.thinning(maps, name)   # 16 iterations: the intermediate map of the rectangle
            w16, st16 = T.thin_batch(maps, method, 16)
            assert np.array_equal(got, w16) and it.tolist() == st16[:, 0].tolist() and conv.tolist() == st16[:, 1].tolist() and conv[0] == 0
            import torch
            one, it1, _ = ctx.thinning(torch.from_numpy(maps[1]).cuda(), method)   # a torch tensor, one map, the method by number
            assert np.array_equal(one[0], want[1]) and it1.tolist() == [want_st[1, 0]]
        with pytest.raises(api.HipCannyError, match="method must be one of"):
            ctx.thinning(maps, "medial")


def test_canny_skeleton_and_canny_components_thin():
    w, h, n = 320, 200, 2
    frames = _scene(w, h, n, 40)
    with api.Context(w, h, 1, n, api.MODE_O) as ctx:
        edges = ctx.canny(frames, 60, 150)
        for close, method in (((api.MORPH_RECT, 3), "zhangsuen"), ((api.MORPH_ELLIPSE, 5), "guohall")):
            closed = M.morph(edges, M.CLOSE, M.structuring_spans(close[0], close[1]))
            want, want_st = T.thin_batch(closed, api.THIN_METHODS[method], 16)
            got, it, conv = ctx.canny_skeleton(frames, 60, 150, close=close, method=method)
            assert np.array_equal(got, want) and it.tolist() == want_st[:, 0].tolist() and conv.tolist() == want_st[:, 1].tolist()
            res = ctx.canny_components(frames, 60, 150, close=close, thin=method)
            ref = ccl_ref.connected_components(want, 8)
            assert np.array_equal(res[0], want) and np.array_equal(res[1], ref[0]) and np.array_equal(res[2], ref[1])
            for f in range(n):
                assert np.array_equal(res[3][f], ref[2][f]) and np.array_equal(res[4][f], ref[3][f])
        blurred = ctx.canny_skeleton(frames, 60, 150, blur=(5, 1.2), max_iterations=8)
        be = ctx.blur_canny(frames, 5, 1.2, 60, 150)
        assert np.array_equal(blurred[0], T.thin_batch(M.morph(be, M.CLOSE, [1, 1, 1]), T.ZHANGSUEN, 8)[0])
        plain = ctx.canny_components(frames, 60, 150)   # with the defaults nothing changes
        assert np.array_equal(plain[0], edges)
        only_thin = ctx.canny_components(frames, 60, 150, thin="guohall")
        assert np.array_equal(only_thin[0], T.thin_batch(edges, T.GUOHALL, 16)[0])


def test_repeatable():
    """The same batch thinned five times on one context gives the same bytes (the removal counts are integer sums)."""
    w, h = 517, 77
    maps = _contents(h, w, 77)
    with api.Context(w, h, 1, len(maps), api.MODE_O) as ctx:
        first = _call(ctx, maps, T.GUOHALL, 40)
        for _ in range(4):
            again = _call(ctx, maps, T.GUOHALL, 40, want=first)
            assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])
