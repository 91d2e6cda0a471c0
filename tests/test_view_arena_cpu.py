"""The view harness itself (tests/view_arena.py), with a numpy stand-in for the kernel: check_output passes for a stand-in
that writes the view and nothing else, and fails for one byte written at column W of a row, in the gap between frames, in
the lead or the trail, and for one wrong pixel inside the view; make_input round-trips the frames in every geometry
family tests/test_gpu_views.py uses."""
import numpy as np
import pytest

import view_arena as VA


def _families(w, h, c):
    """(name, in_pitch, in_frame_stride, in_base_off, out_pitch, out_frame_stride, out_base_off) as test_gpu_views draws them."""
    rb, w8 = w * c, VA.round_up(w, 8)
    p4i, p4o = w8 * c + 4, w8 + 4
    gmi, gmo = VA.round_up(rb, 512) + 512, VA.round_up(w, 512)
    roi_i, roi_o = VA.round_up(rb + 4 + 37 * c, 4) + 64, VA.round_up(w + 8 + 21, 4) + 32
    return [
        ("T", rb, rb * h, 0, w, w * h, 0),
        ("P4", p4i, p4i * h + 20, 4, p4o, p4o * h + 20, 12),
        ("GM", gmi, gmi * h, 0, gmo, gmo * h, 0),
        ("ROI", roi_i, roi_i * (h + 9), 3 * roi_i + 4 + 16 * c, roi_o, roi_o * (h + 5), 2 * roi_o + 8),
        ("MIX", p4i, p4i * h + 20, 4, w, w * h, 0),
        ("ODD", rb + 1, (rb + 1) * h + 3, 1, w + 3, (w + 3) * h + 1, 3),
    ]


def _standin(frames):
    """The "operation" of the stand-in kernel: any deterministic map to 0 / 255 bytes, (n, H, W)."""
    a = frames if frames.ndim == 3 else frames.max(axis=-1)
    return np.where(a > 100, 255, 0).astype(np.uint8)


def _standin_kernel(in_arena, gi, out_arena, go, c):
    """Reads the input view, writes the output view -- and only the view."""
    src = VA.read_view(in_arena, gi)
    frames = src if c == 1 else src.reshape(gi.n, gi.rows, -1, c)
    out_arena[go.index()] = _standin(frames)


CASES = [(w, h, c, n) for w in (1, 5, 29, 241, 640) for h in (1, 5, 37) for c in (1, 3) for n in (1, 3)]


@pytest.mark.parametrize("fill", VA.FILLS)
def test_make_input_round_trips(fill):
    rng = np.random.default_rng(1)
    for w, h, c, n in CASES:
        frames = rng.integers(0, 256, (n, h, w) if c == 1 else (n, h, w, c), dtype=np.uint8)
        for name, ip, ifs, ioff, _, _, _ in _families(w, h, c):
            arena, off = VA.make_input(frames, ip, ifs, ioff, fill, seed=3)
            g = VA.input_geometry(frames, ip, ifs, ioff)
            assert off == g.offset == g.lead + ioff and arena.size == g.size and arena.dtype == np.uint8, name
            assert g.lead >= ip + 64 and g.trail >= ip + 64
            assert np.array_equal(VA.read_view(arena, g).reshape(frames.shape), frames), (name, w, h, c, n)
            # the documented address of every row, spelled out
            for f in (0, n - 1):
                for r in (0, h - 1):
                    a = g.lead + ioff + f * ifs + r * ip
                    assert np.array_equal(arena[a:a + w * c], frames[f, r].reshape(-1)), (name, f, r)
            # and nothing but the view depends on the frames
            other, _ = VA.make_input(255 - frames, ip, ifs, ioff, fill, seed=3)
            assert np.array_equal(arena[~g.inside()], other[~g.inside()]), name
            if fill == "ff":
                assert (arena[~g.inside()] == 255).all()


def test_make_input_int16_frames():
    rng = np.random.default_rng(2)
    for shape in ((2, 5, 29), (3, 4, 7, 3)):
        dx = rng.integers(-32768, 32768, shape).astype(np.int16)
        rb = 2 * int(np.prod(shape[2:]))
        pitch = rb + 2   # = 0 mod 4 or 2 mod 4: the gradient entry asks for even values only
        arena, off = VA.make_input(dx, pitch, pitch * shape[1] + 6, 2, "random")
        g = VA.input_geometry(dx, pitch, pitch * shape[1] + 6, 2)
        assert g.row_bytes == rb and off == g.lead + 2
        assert np.array_equal(VA.read_view(arena, g).reshape(-1).view(np.int16).reshape(shape), dx)


def test_make_output_pattern_and_arguments():
    arena, g = VA.make_output(3, 7, 29, 36, 36 * 7 + 20, 12, seed=5)
    assert arena.size == g.size and arena.min() >= 1 and arena.max() <= 254
    assert np.array_equal(arena, VA.make_output(3, 7, 29, 36, 36 * 7 + 20, 12, seed=5)[0])
    for bad in (dict(pitch=28), dict(frame_stride=36 * 7 - 1), dict(lead=36 + 63), dict(trail=10), dict(base_off=-1)):
        kw = dict(n=3, rows=7, row_bytes=29, pitch=36, frame_stride=36 * 7 + 20, base_off=12)
        kw.update(bad)
        with pytest.raises(ValueError):
            VA.make_output(**kw)


@pytest.mark.parametrize("w,h,c,n", [(5, 5, 1, 3), (29, 2, 3, 1), (241, 37, 1, 3), (640, 5, 3, 3), (1, 1, 1, 1)])
def test_check_output_with_standin_kernel(w, h, c, n):
    rng = np.random.default_rng(w + h)
    frames = rng.integers(0, 256, (n, h, w) if c == 1 else (n, h, w, c), dtype=np.uint8)
    want = _standin(frames)
    for name, ip, ifs, ioff, op, ofs, ooff in _families(w, h, c):
        in_arena, _ = VA.make_input(frames, ip, ifs, ioff, "random", seed=9)
        gi = VA.input_geometry(frames, ip, ifs, ioff)
        before, go = VA.make_output(n, h, w, op, ofs, ooff, seed=4)
        after = before.copy()
        _standin_kernel(in_arena, gi, after, go, c)
        VA.check_output(after, before, go, want, name)   # the correct stand-in passes

        def fails(off, value, needle):
            broken = after.copy()
            broken[off] = value
            with pytest.raises(AssertionError) as ei:
                VA.check_output(broken, before, go, want, name)
            assert needle in str(ei.value), str(ei.value)
            return str(ei.value)

        def other(off):   # a value that differs from the byte before the run (guards) / from the wanted pixel (view)
            return (int(after[off]) + 1) % 256

        starts = go.row_starts()
        # one byte at column W of one row (only where the pitch leaves room: a tight row's column W is the next row's pixel)
        f, r = n - 1, h // 2
        if op > w:
            msg = fails(starts[f, r] + w, other(starts[f, r] + w), "OUTSIDE")
            assert f"(frame {f}, row {r}, col {w})" in msg and "1 bytes" in msg
            fails(starts[f, r] + op - 1, 0, "OUTSIDE")          # the last padding byte of the row
        if ofs > op * h:                                          # the gap between frames / behind the last frame
            msg = fails(go.offset + op * h, 255, "OUTSIDE")
            assert f"(frame 0, row {h}, col 0)" in msg
            fails(go.offset + (n - 1) * ofs + op * h + (ofs - op * h) - 1, 0, "OUTSIDE")
        fails(0, 0, "OUTSIDE")                                    # lead: first byte, and the byte just before the view
        msg = fails(go.offset - 1, 255, "OUTSIDE")
        assert "row -1" in msg
        fails(go.size - 1, 0, "OUTSIDE")                          # trail: last byte, and the first one behind the view
        fails(starts[n - 1, h - 1] + w, other(starts[n - 1, h - 1] + w), "OUTSIDE")
        # one pixel inside the view
        msg = fails(starts[f, r] + w - 1, other(starts[f, r] + w - 1), "inside the view")
        assert f"(frame {f}, row {r}, col {w - 1})" in msg and "OUTSIDE" not in msg
        fails(starts[0, 0], other(starts[0, 0]), "inside the view")


def test_check_output_reports_both_kinds_and_counts():
    before, g = VA.make_output(2, 4, 8, 12, 60, 4, seed=1)
    want = np.zeros((2, 4, 8), np.uint8)
    after = before.copy()
    after[g.index()] = want
    VA.check_output(after, before, g, want)
    after[g.row_starts()[1, 2] + 8:g.row_starts()[1, 2] + 12] = 0   # a store one group too wide: the 4 padding bytes of a row
    after[g.row_starts()[0, 0] + 3] = 255
    with pytest.raises(AssertionError) as ei:
        VA.check_output(after, before, g, want, "wide store")
    msg = str(ei.value)
    assert "wide store" in msg and "1 of 64 bytes inside" in msg and "4 bytes OUTSIDE" in msg
    assert "(frame 1, row 2, col 8)" in msg and "(frame 0, row 0, col 3): got 255, want 0" in msg
    with pytest.raises(ValueError):
        VA.check_output(after[:-1], before, g, want)
    with pytest.raises(ValueError):
        VA.check_output(after, before, g, want[:1])
