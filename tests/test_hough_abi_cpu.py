"""hc_hough_tables through ctypes without a GPU (the library loads without one): geometry and tables equal, bit for bit, those of
tests/hough_ref.py; its refusals return HC_E_ARG and write nothing.  hc_hough_lines_device refuses a null context."""
import ctypes as C
import math

import numpy as np
import pytest

import hough_ref as R
from cudacam_amd import api
from test_hough_plan_cpu import TABLE_ARGS

FP = C.POINTER(C.c_float)
SENTINEL = np.float32(-77.0)


def _raw(args, cap, tables=True, geo=True, only=None):
    lib = api.load_library()
    na, nr = C.c_int(-7), C.c_int(-7)
    tabs = [np.full(max(cap, 1) + 2, SENTINEL, np.float32) for _ in range(3)]
    ptrs = [t.ctypes.data_as(FP) if tables and (only is None or k in only) else None for k, t in enumerate(tabs)]
    w, h, rho, theta, lo, hi = args
    rc = lib.hc_hough_tables(int(w), int(h), float(rho), float(theta), float(lo), float(hi), C.byref(na) if geo else None, C.byref(nr) if geo else None, *ptrs, cap)
    return rc, na.value, nr.value, tabs


@pytest.mark.parametrize("args", TABLE_ARGS)
def test_tables_equal_the_restatement(args):
    want_geo = R.geometry(*args)
    rc, na, nr, tabs = _raw(args, 0, tables=False)
    assert rc == 0 and (na, nr) == want_geo
    rc, na, nr, tabs = _raw(args, na)
    assert rc == 0 and (na, nr) == want_geo
    for got, want in zip(tabs, R.tables(*args)):
        assert np.array_equal(got[:na].view(np.uint32), want.view(np.uint32))
        assert (got[na:] == SENTINEL).all()
    py = api.hough_tables(*args)
    assert py[:2] == want_geo and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(py[2:], R.tables(*args)))


def test_refusals_write_nothing():
    good = (64, 48, 1.0, math.pi / 4, 0.0, math.pi)   # four angles
    inf, nan = math.inf, math.nan
    bad = [(0, 48) + good[2:], (64, 0) + good[2:], (-1, 48) + good[2:]]
    bad += [good[:2] + (v,) + good[3:] for v in (0.0, -1.0, inf, nan)]
    bad += [good[:3] + (v,) + good[4:] for v in (0.0, -0.1, inf, nan)]
    bad += [good[:4] + (v, math.pi) for v in (inf, -inf, nan, 4.0)]       # 4.0: above max_theta
    bad += [good[:5] + (v,) for v in (inf, nan, -1.0)]
    bad += [(64, 48, 1e-6, math.pi / 4, 0.0, math.pi),                    # a row beyond LDS
            (1, 1, 1.0, 1e-9, 0.0, math.pi)]                              # 2^31 cells
    for args in bad:
        rc, na, nr, tabs = _raw(args, 8)
        assert rc == -1 and (na, nr) == (-7, -7) and all((t == SENTINEL).all() for t in tabs), args
        assert "hc_hough_tables" in api.last_error()
    for kw in (dict(cap=3), dict(cap=0), dict(cap=8, only=(0,)), dict(cap=8, only=(0, 2)), dict(cap=8, geo=False)):
        cap = kw.pop("cap")
        rc, na, nr, tabs = _raw(good, cap, **kw)
        assert rc == -1 and (na, nr) == (-7, -7) and all((t == SENTINEL).all() for t in tabs), kw
    rc, na, nr, tabs = _raw(good, 4)
    assert rc == 0 and (na, nr) == (4, 225)
    with pytest.raises(api.HipCannyError, match="error -1"):
        api.hough_tables(64, 48, 0.0, 1.0)


def test_the_device_entry_refuses_a_null_context():
    for lib in (api.load_library(), api.load_library(legacy=True)):
        assert lib.hc_hough_lines_device(None, 8, 8, 1, 1, 1.0, 0.1, 1, 0.0, 3.0, 8, 8, 1) == -1
