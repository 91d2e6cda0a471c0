"""The C ABI of the circle entries without a GPU: hc_hough_circle_geometry through ctypes equals the numpy restatement and refuses
as the header says, writing nothing; the header's argument lists of both entries match the argtypes api.py gives ctypes; both
symbols are exported by both libraries; hc_hough_circles_device refuses a null context under its own name, and the test library
refuses it altogether."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

import hough_circles_ref as HC
from cudacam_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["hc_hough_circles_device", "hc_hough_circle_geometry"]
GEOMETRIES = [(w, h, dp, md, 3, 40) for w, h in ((1, 1), (9, 7), (65, 64), (200, 150), (1920, 1080)) for dp in (1.0, 1.5, 2.0, 7.3) for md in (0.0, 1.0, 2.5 * dp, 1e3)]
DEVICE_ARGS = (16, 16, 100, 16, 16, 128, 128 * 48, 1, 1.0, 5.0, 10, 3, 20, 4096, 16, 16, 4)   # every pointer non-null and aligned


@pytest.fixture(scope="module")
def lib():
    build.build()
    return api.load_library()


@pytest.mark.parametrize("args", GEOMETRIES)
def test_geometry_equals_the_restatement(lib, args):
    assert api.hough_circle_geometry(*args) == HC.geometry(*args)


def test_geometry_refusals_write_nothing(lib):
    aw, ah, d2 = C.c_int(-7), C.c_int(-7), C.c_longlong(-7)
    out = (C.byref(aw), C.byref(ah), C.byref(d2))
    good = (64, 48, 2.0, 5.0, 3, 20)
    bad = [(good, (None, out[1], out[2])), (good, (out[0], None, out[2])), (good, (out[0], out[1], None))]
    bad += [(g, out) for g in ((0, 48, 2.0, 5.0, 3, 20), (64, 0, 2.0, 5.0, 3, 20), (64, 48, 2.0, 5.0, 0, 20), (64, 48, 2.0, 5.0, 21, 20), (64, 48, 2.0, 5.0, 1, 4095),
                               (64, 48, 2.0, 5.0, 3, (1 << 20) - 64), (64, 48, 1e300, 5.0, 3, 20))]
    bad += [((64, 48, v, 5.0, 3, 20), out) for v in (0.5, 0.0, -2.0, math.inf, math.nan)]
    bad += [((64, 48, 2.0, v, 3, 20), out) for v in (-1.0, math.inf, -math.inf, math.nan)]
    for geo, ptrs in bad:
        assert lib.hc_hough_circle_geometry(*geo, *ptrs) == -1, geo
        assert "hc_hough_circle_geometry" in api.last_error()
        assert (aw.value, ah.value, d2.value) == (-7, -7, -7), geo
    assert lib.hc_hough_circle_geometry(*good, *out) == 0 and (aw.value, ah.value, d2.value) == (32, 24, 7)


def _ctype_of(decl):
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S).strip()
    if "*" in decl:
        base = decl.split("*")[0].strip()
        return {"int": C.POINTER(C.c_int), "long long": C.POINTER(C.c_longlong)}.get(base, C.c_void_p)   # hc_ctx *, void *, const void *
    return {"int": C.c_int, "size_t": C.c_size_t, "double": C.c_double}[decl.rsplit(" ", 1)[0].strip()]


@pytest.mark.parametrize("name", NAMES)
def test_header_arguments_match_ctypes(lib, name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hipcanny.h")).read(), flags=re.S)
    body = re.search(r"\bint " + name + r"\s*\((.*?)\);", hdr, re.S).group(1)
    want = [_ctype_of(a) for a in body.split(",")]
    assert getattr(lib, name).argtypes == want
    assert len(want) == {"hc_hough_circles_device": 18, "hc_hough_circle_geometry": 9}[name]


def test_both_symbols_are_exported_by_both_libraries(lib):
    assert set(NAMES) <= set(api.ABI_SYMBOLS)
    for path in (api.LIB_PATH, build.build_legacy()):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        assert set(NAMES) <= exported, path


def test_a_null_context_is_refused_under_the_entry_s_name(lib):
    assert lib.hc_hough_circles_device(None, *DEVICE_ARGS) == -1
    assert "hc_hough_circles_device" in api.last_error()


def test_the_test_library_refuses_the_device_entry_and_gives_the_geometry():
    build.build_legacy()
    legacy = api.load_library(legacy=True)
    assert legacy.hc_hough_circles_device(None, *DEVICE_ARGS) == -1
    assert "hc_hough_circles_device: not part of the test library" in legacy.hc_last_error().decode()
    aw, ah, d2 = C.c_int(0), C.c_int(0), C.c_longlong(0)
    assert legacy.hc_hough_circle_geometry(65, 31, 2.0, 5.0, 3, 20, C.byref(aw), C.byref(ah), C.byref(d2)) == 0
    assert (aw.value, ah.value, d2.value) == HC.geometry(65, 31, 2.0, 5.0, 3, 20) == (33, 16, 7)
