"""The C ABI of the segment entries without a GPU: hc_hough_walk_tables through ctypes equals the numpy restatement bit for bit and
refuses as the header says, writing nothing; the header's argument lists of both entries match the argtypes api.py gives ctypes;
both symbols are exported by both libraries; hc_hough_segments_device refuses a null context under its own name."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import hough_segments_ref as S
from cudacam_amd import api, build
from test_hough_plan_cpu import TABLE_ARGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI = math.pi
FP, IP = C.POINTER(C.c_float), C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return api.load_library()


@pytest.mark.parametrize("args", TABLE_ARGS)
def test_walk_tables_equal_the_restatement(lib, args):
    w, h, rho, theta, lo, hi = args
    numangle, major, slope, scale = api.hough_walk_tables(*args)
    want = S.walk_tables(w, h, rho, theta, lo, hi)
    assert numangle == len(want[0]) and major.dtype == np.int32 and slope.dtype == np.float32 and scale.dtype == np.float32
    assert np.array_equal(major, want[0])
    assert np.array_equal(slope.view(np.uint32), want[1].view(np.uint32)) and np.array_equal(scale.view(np.uint32), want[2].view(np.uint32))


def test_walk_tables_refusals_write_nothing(lib):
    major, slope, scale = np.full(8, -77, np.int32), np.full(8, -77, np.float32), np.full(8, -77, np.float32)
    mj, sl, sc = major.ctypes.data_as(IP), slope.ctypes.data_as(FP), scale.ctypes.data_as(FP)
    na = C.c_int(-7)
    good = (64, 48, 1.0, PI / 4, 0.0, PI)
    bad = [(good, (None, mj, sl, sc, 8)), (good, (C.byref(na), mj, None, sc, 8)), (good, (C.byref(na), None, sl, sc, 8)), (good, (C.byref(na), mj, sl, None, 8)),
           (good, (C.byref(na), mj, sl, sc, 3)), ((0, 48, 1.0, PI / 4, 0.0, PI), (C.byref(na), mj, sl, sc, 8)), ((64, 0, 1.0, PI / 4, 0.0, PI), (C.byref(na), mj, sl, sc, 8)),
           ((64, 48, 1.0, PI / 4, 1.0, 0.5), (C.byref(na), mj, sl, sc, 8)), ((64, 48, 1e-6, PI / 4, 0.0, PI), (C.byref(na), mj, sl, sc, 8))]
    bad += [((64, 48, v, PI / 4, 0.0, PI), (C.byref(na), mj, sl, sc, 8)) for v in (0.0, -1.0, math.inf, math.nan)]
    bad += [((64, 48, 1.0, v, 0.0, PI), (C.byref(na), mj, sl, sc, 8)) for v in (0.0, -1.0, math.inf, math.nan)]
    bad += [((64, 48, 1.0, PI / 4, v, PI), (C.byref(na), mj, sl, sc, 8)) for v in (math.inf, -math.inf, math.nan)]
    for geo, rest in bad:
        assert lib.hc_hough_walk_tables(*geo, *rest) == -1, (geo, rest[4])
        assert "hc_hough_walk_tables" in api.last_error()
        assert na.value == -7 and (major == -77).all() and (slope == -77).all() and (scale == -77).all(), (geo, rest[4])
    assert lib.hc_hough_walk_tables(*good, C.byref(na), None, None, None, 0) == 0 and na.value == 4 and (major == -77).all()   # numangle only
    assert lib.hc_hough_walk_tables(*good, C.byref(na), mj, sl, sc, 4) == 0
    assert major[:4].tolist() == [1, 0, 0, 1] and (major[4:] == -77).all() and (slope[4:] == -77).all() and (scale[4:] == -77).all()


def _ctype_of(decl):
    decl = re.sub(r"/\*.*?\*/", "", decl).strip()
    if "*" in decl:
        base = decl.split("*")[0].strip()
        return {"int": C.POINTER(C.c_int), "int32_t": C.POINTER(C.c_int32), "float": C.POINTER(C.c_float)}.get(base, C.c_void_p)   # hc_ctx *, void *, const void *
    return {"int": C.c_int, "size_t": C.c_size_t, "double": C.c_double}[decl.rsplit(" ", 1)[0].strip()]


@pytest.mark.parametrize("name", ["hc_hough_segments_device", "hc_hough_walk_tables"])
def test_header_arguments_match_ctypes(lib, name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hipcanny.h")).read(), flags=re.S)
    body = re.search(r"\bint " + name + r"\s*\((.*?)\);", hdr, re.S).group(1)
    want = [_ctype_of(a) for a in body.split(",")]
    assert getattr(lib, name).argtypes == want
    assert len(want) == {"hc_hough_segments_device": 17, "hc_hough_walk_tables": 11}[name]


def test_both_symbols_are_exported_by_both_libraries(lib):
    assert "hc_hough_segments_device" in api.ABI_SYMBOLS and "hc_hough_walk_tables" in api.ABI_SYMBOLS
    for path in (api.LIB_PATH, build.build_legacy()):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        assert {"hc_hough_segments_device", "hc_hough_walk_tables"} <= exported, path


def test_a_null_context_is_refused_under_the_entry_s_name(lib):
    assert lib.hc_hough_segments_device(None, 16, 64, 64 * 48, 16, 16, 4, 1, 1.0, PI / 180, 0.0, PI, 10, 2, 16, 16, 4) == -1
    assert "hc_hough_segments_device" in api.last_error()


def test_the_test_library_refuses_the_device_entry_and_gives_the_tables():
    build.build_legacy()
    legacy = api.load_library(legacy=True)
    assert legacy.hc_hough_segments_device(None, 16, 64, 64 * 48, 16, 16, 4, 1, 1.0, PI / 180, 0.0, PI, 10, 2, 16, 16, 4) == -1
    assert "hc_hough_segments_device: not part of the test library" in legacy.hc_last_error().decode()
    na = C.c_int(0)
    major, slope, scale = np.empty(4, np.int32), np.empty(4, np.float32), np.empty(4, np.float32)
    assert legacy.hc_hough_walk_tables(64, 48, 1.0, PI / 4, 0.0, PI, C.byref(na), major.ctypes.data_as(IP), slope.ctypes.data_as(FP), scale.ctypes.data_as(FP), 4) == 0
    want = S.walk_tables(64, 48, 1.0, PI / 4)
    assert na.value == 4 and np.array_equal(major, want[0]) and np.array_equal(slope.view(np.uint32), want[1].view(np.uint32)) and np.array_equal(scale.view(np.uint32), want[2].view(np.uint32))
