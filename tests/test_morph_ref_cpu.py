"""tests/morph_ref.py -- the numpy restatement of hc_morphology_device -- anchored without a GPU: against scipy.ndimage's grey
morphology (which reflects the footprint for dilation only, so the dilation is given the flipped one), the compound operations
against compositions, the orientation of a vertically asymmetric element by its impulse response, the three pinned ellipse
tables, iterated RECTs against larger RECTs, and the agreement of the header, api.py and the legacy library's refusal."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cudacam_amd import api, build
import morph_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPANS = [[1, 0, -1], [0, 2, 2, 2, 0], [-1, 0, 3, 1, 2, 0, 3], [0, -1, -1], [1, 1, 1], [0, 0, 2, 0, 0], [0, 2, 3, 3, 3, 2, 0], [-1, -1, -1, -1, -1, -1, 2]]
SIZES = [(1, 1), (2, 9), (9, 2), (13, 11)]


@pytest.mark.parametrize("spans", SPANS, ids=[str(s) for s in SPANS])
def test_against_scipy(spans):
    ndi = pytest.importorskip("scipy.ndimage")
    fp = M.footprint(spans)
    for h, w in SIZES:
        a = np.random.default_rng(h * 100 + w).integers(0, 256, (h, w), dtype=np.uint8)
        want_d = ndi.grey_dilation(a, footprint=fp[::-1, ::-1], mode="constant", cval=0)
        want_e = ndi.grey_erosion(a, footprint=fp, mode="constant", cval=255)
        assert np.array_equal(M.dilate(a[None], spans)[0], want_d), (spans, h, w)
        assert np.array_equal(M.erode(a[None], spans)[0], want_e), (spans, h, w)
        c3 = np.stack([a, 255 - a, a[::-1, ::-1]], -1)   # channels are independent
        got = M.dilate(c3[None], spans)[0]
        for ch in range(3):
            assert np.array_equal(got[..., ch], ndi.grey_dilation(c3[..., ch], footprint=fp[::-1, ::-1], mode="constant", cval=0))


def test_loop_restatement():
    """The definition, pixel by pixel."""
    rng = np.random.default_rng(5)
    for spans in SPANS:
        k = len(spans)
        a = rng.integers(0, 256, (6, 7), dtype=np.uint8)
        d, e = np.zeros_like(a), np.zeros_like(a)
        for y in range(6):
            for x in range(7):
                vals = [int(a[y + j - k // 2, x + dx]) for j, s in enumerate(spans) for dx in range(-s, s + 1)
                        if 0 <= y + j - k // 2 < 6 and 0 <= x + dx < 7]
                d[y, x] = max(vals, default=0)
                e[y, x] = min(vals, default=255)
        assert np.array_equal(M.dilate(a[None], spans)[0], d) and np.array_equal(M.erode(a[None], spans)[0], e), spans


def test_compound_ops_are_compositions():
    a = np.random.default_rng(1).integers(0, 256, (2, 12, 15, 3), dtype=np.uint8)
    for spans in SPANS:
        d, e = M.dilate(a, spans), M.erode(a, spans)
        assert np.array_equal(M.morph(a, M.OPEN, spans, 3), M.dilate(e, spans))
        assert np.array_equal(M.morph(a, M.CLOSE, spans, 3), M.erode(d, spans))
        # the erosion exceeds the dilation only where the window holds no position of the frame: 0 against 255, gradient 0
        assert ((d >= e) | ((d == 0) & (e == 255))).all()
        assert np.array_equal(M.morph(a, M.GRADIENT, spans, 3), np.clip(d.astype(int) - e, 0, 255).astype(np.uint8))
        assert np.array_equal(M.morph(a, M.DILATE, spans), d) and np.array_equal(M.morph(a, M.ERODE, spans), e)


def test_orientation_by_impulse_response():
    """spans [1, 0, -1]: the element's top row is 3 wide, its middle row the anchor alone.  out(y, x) takes src(y - 1, x - 1 .. x
    + 1) and src(y, x), so an impulse at (4, 4) spreads DOWN into row 5, three wide -- not up (that would be the reflected element)."""
    a = np.zeros((1, 9, 9), np.uint8)
    a[0, 4, 4] = 200
    d = M.dilate(a, [1, 0, -1])[0]
    assert sorted(map(tuple, np.argwhere(d))) == [(4, 4), (5, 3), (5, 4), (5, 5)]
    e = M.erode(255 - a, [1, 0, -1])[0]
    assert sorted(map(tuple, np.argwhere(e != 255))) == [(4, 4), (5, 3), (5, 4), (5, 5)]
    # an element of its top row only, at row 0: no position inside the frame
    top = [1, -1, -1]
    r = np.random.default_rng(2).integers(1, 255, (1, 3, 5), dtype=np.uint8)
    assert (M.dilate(r, top)[0, 0] == 0).all() and (M.erode(r, top)[0, 0] == 255).all()


def test_pinned_structuring_elements():
    assert M.structuring_spans(M.ELLIPSE, 3) == [0, 1, 0] == M.structuring_spans(M.CROSS, 3)
    assert M.structuring_spans(M.ELLIPSE, 5) == [0, 2, 2, 2, 0]
    assert M.structuring_spans(M.ELLIPSE, 7) == [0, 2, 3, 3, 3, 2, 0]
    for k in M.KSIZES:
        assert M.structuring_spans(M.RECT, k) == [k // 2] * k
        assert M.structuring_spans(M.CROSS, k) == [k // 2 if j == k // 2 else 0 for j in range(k)]


def test_library_structuring_element_matches():
    """hc_structuring_element (a host function of both libraries) gives the same tables; refusals write nothing."""
    build.build()
    for lib in (api.load_library(), api.load_library(legacy=True)):
        for shape in M.SHAPES:
            for k in M.KSIZES:
                buf = (C.c_int8 * 8)(*([77] * 8))
                assert lib.hc_structuring_element(shape, k, buf) == 0
                assert list(buf[:k]) == M.structuring_spans(shape, k) and list(buf[k:]) == [77] * (8 - k)
        buf = (C.c_int8 * 8)(*([77] * 8))
        for shape, k in ((-1, 3), (3, 3), (0, 4), (0, 9), (2, 0)):
            assert lib.hc_structuring_element(shape, k, buf) == -1 and list(buf) == [77] * 8
            assert "hc_structuring_element" in lib.hc_last_error().decode()
        assert lib.hc_structuring_element(0, 3, None) == -1
    assert api.structuring_element(api.MORPH_ELLIPSE, 7) == [0, 2, 3, 3, 3, 2, 0]


def test_iterated_rect_is_a_larger_rect():
    a = np.random.default_rng(3).integers(0, 256, (1, 17, 19), dtype=np.uint8)
    for n in (1, 2, 3):
        big = [n] * (2 * n + 1)
        for op in (M.ERODE, M.DILATE, M.OPEN, M.CLOSE, M.GRADIENT):
            assert np.array_equal(M.morph_iterated(a, op, [1, 1, 1], n), M.morph(a, op, big)), (n, op)


def test_header_api_and_enums_agree():
    hdr = open(os.path.join(ROOT, "include", "hipcanny.h")).read()
    ops = re.search(r"enum \{ HC_MORPH_ERODE = 0, HC_MORPH_DILATE = 1, HC_MORPH_OPEN = 2, HC_MORPH_CLOSE = 3, HC_MORPH_GRADIENT = 4 \};", hdr)
    shapes = re.search(r"enum \{ HC_MORPH_RECT = 0, HC_MORPH_CROSS = 1, HC_MORPH_ELLIPSE = 2 \};", hdr)
    assert ops and shapes
    assert (api.MORPH_ERODE, api.MORPH_DILATE, api.MORPH_OPEN, api.MORPH_CLOSE, api.MORPH_GRADIENT) == M.OPS == (0, 1, 2, 3, 4)
    assert (api.MORPH_RECT, api.MORPH_CROSS, api.MORPH_ELLIPSE) == M.SHAPES == (0, 1, 2)
    assert "hc_morphology_device" in api.ABI_SYMBOLS and "hc_structuring_element" in api.ABI_SYMBOLS
    assert re.search(r"int hc_morphology_device\(hc_ctx \*ctx, const void \*d_in, size_t in_pitch, size_t in_frame_stride, void \*d_out, size_t out_pitch,\s*size_t out_frame_stride, int nframes, int channels, int op, int ksize, const int8_t \*spans", hdr)
    assert re.search(r"int hc_structuring_element\(int shape, int ksize, int8_t \*spans\);", hdr)
    assert "tests/morph_ref.py" in hdr and "not pinned against a build of OpenCV" in hdr


def test_legacy_library_refuses_the_entry():
    build.build()
    lib = api.load_library(legacy=True)
    spans = (C.c_int8 * 3)(1, 1, 1)
    assert lib.hc_morphology_device(None, None, 0, 0, None, 0, 0, 1, 1, 1, 3, spans) == -1
    assert lib.hc_last_error().decode() == "hc_morphology_device: not part of the test library"
