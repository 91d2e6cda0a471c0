"""hc_edge_points_device without a GPU.

* the numpy restatement tests/edge_points_ref.py against a literal written out by hand and against a double loop;
* include/hipcanny.h, api.py and the built product library agree on the entry (declared, bound, exported, its three kernels in
  the code object), and a null context is HC_E_ARG before any device is touched -- the test that fails without the feature;
* libhipcanny_legacy.so exports the entry and refuses it.
The work split is k_hist256's rule (hist_chunk_rows, canny_params.h): no new function, nothing more to drive here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import edge_points_ref as R
from cudacam_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_on_a_literal():
    m = np.array([[0, 255, 0, 0, 128],
                  [0, 0, 0, 0, 0],
                  [1, 0, 255, 255, 0]], np.uint8)
    want = [(1, 0), (4, 0), (0, 2), (2, 2), (3, 2)]   # (x, y): row 0 left to right, then row 2
    assert R.count(m) == 5
    p = R.points(m)
    assert p.dtype == np.int32 and p.shape == (5, 2) and p.flags["C_CONTIGUOUS"]
    assert [tuple(int(v) for v in q) for q in p] == want
    assert [tuple(int(v) for v in q) for q in R.points(m, 3)] == want[:3]
    assert R.points(m, 0).shape == (0, 2) and R.points(m, 9).shape == (5, 2)
    assert R.points(np.zeros((3, 5), np.uint8)).shape == (0, 2)
    counts, lists = R.edge_points(np.stack([m, np.zeros_like(m), m]), 4)
    assert counts.dtype == np.uint32 and counts.tolist() == [5, 0, 5]
    assert [len(q) for q in lists] == [4, 0, 4]


def test_restatement_equals_a_double_loop():
    rng = np.random.default_rng(20261019)
    for h, w, density in ((1, 1, 1.0), (1, 7, 0.5), (7, 1, 0.5), (9, 13, 0.3), (16, 64, 0.02), (5, 5, 0.0)):
        m = np.where(rng.random((h, w)) < density, rng.integers(1, 256, (h, w)), 0).astype(np.uint8)
        brute = [(x, y) for y in range(h) for x in range(w) if m[y, x] != 0]
        assert R.count(m) == len(brute)
        assert [tuple(int(v) for v in q) for q in R.points(m)] == brute
        for cap in (0, 1, len(brute) // 2, len(brute), len(brute) + 3):
            assert [tuple(int(v) for v in q) for q in R.points(m, cap)] == brute[:cap]


def _args(hdr, name):
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)   # (the declaration's own comments hold commas and semicolons)
    m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
    assert m, f"include/hipcanny.h does not declare {name}"
    body = m.group(1).replace("\n", " ")
    return [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*").strip() for a in body.split(",")]


def test_entry_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "hipcanny.h")).read()
    assert _args(hdr, "hc_edge_points_device") == ["hc_ctx*", "const void*", "size_t", "size_t", "int", "void*", "void*", "size_t"]
    assert "hc_edge_points_device" in api.ABI_SYMBOLS
    for meth in ("edge_points_device", "edge_points", "canny_points"):
        assert callable(getattr(api.Context, meth))
    build.build()
    lib = api.load_library()
    assert len(lib.hc_edge_points_device.argtypes) == 8
    out = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0
    assert re.search(r"\bT hc_edge_points_device\b", out.stdout)
    blob = open(api.LIB_PATH, "rb").read()
    for kernel in (b"k_edge_count", b"k_edge_scan", b"k_edge_emit"):
        assert kernel in blob, kernel
    # argument errors, before any device is touched: a null context, whatever else is passed
    buf = (C.c_uint32 * 4)()
    assert lib.hc_edge_points_device(None, None, 0, 0, 1, None, None, 0) == -1
    assert lib.hc_edge_points_device(None, C.addressof(buf), 4, 4, 1, C.addressof(buf), None, 0) == -1
    assert b"hc_edge_points_device" in lib.hc_last_error()


def test_the_test_library_refuses_the_entry():
    assert "edge_points.hip" in build.SOURCES and "edge_points.hip" not in build.LEGACY_SOURCES
    build.build_legacy()
    lib = api.load_library(legacy=True)
    buf = (C.c_uint32 * 4)()
    assert lib.hc_edge_points_device(None, C.addressof(buf), 4, 4, 1, C.addressof(buf), None, 0) == -1
    assert b"not part of the test library" in lib.hc_last_error()
    blob = open(api.LEGACY_LIB_PATH, "rb").read()
    assert b"k_edge_emit" not in blob
