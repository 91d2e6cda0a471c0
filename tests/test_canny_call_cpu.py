"""hc_canny_device without a GPU: the ABI (header, api.py, the built library), its threshold function and its plans.

* include/hipcanny.h declares hc_canny_device and the forms HC_FORM_O_APERTURE7 = 8 / HC_FORM_O_SCHARR = 9; api.py agrees;
  libhipcanny.so exports the symbol.
* canny_call_thresholds (cudacam_amd/csrc/host_plan.h), compiled with g++ under ASan + UBSan into tests/cpp/
  canny_call_driver.cpp, equals canny_o_ext_ref.thresholds(low / s, high / s, l2) -- s = 16 at aperture 7, 1 elsewhere -- on a
  grid of integers, halves, values just below and above multiples of 16, 0, swapped pairs, values beyond 32767 and beyond
  16 * 32767, both L2 settings, all four apertures; the values the kernels compare are those, the L1 ones clamped to 32767
  (which no L1 magnitude of a u8 source reaches: 24480 at most).  Negative and NaN thresholds are refused.
* the planner: apertures 7 / -1 plan to forms 8 / 9 for 1 and 3 channels, plain and pipelined, cut like aperture 5 on the
  same input; aperture-5 and gradient plans made beside them are what they are with the new fields at their defaults."""
import math
import os
import re
import subprocess

import pytest

import canny_o_ext_ref as X
from cudacam_amd import api, build
from test_sanitizers import ENV, ROOT, SAN, _cc

DRIVER = os.path.join(ROOT, "tests", "cpp", "canny_call_driver.cpp")
APERTURES = (3, 5, 7, -1)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("canny_call") / "canny_call_driver")
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-o", exe, DRIVER])
    return exe


def test_header_api_and_library_agree():
    hdr = open(os.path.join(ROOT, "include", "hipcanny.h")).read()
    m = re.search(r"int\s+hc_canny_device\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/hipcanny.h does not declare hc_canny_device"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert [re.sub(r"\s*\w+$", "", a).replace(" *", "*").strip() for a in args] == [
        "hc_ctx*", "const void*", "size_t", "size_t", "void*", "size_t", "size_t", "int", "double", "double", "int", "int"]
    assert re.search(r"\bHC_FORM_O_APERTURE7\s*=\s*8\b", hdr) and re.search(r"\bHC_FORM_O_SCHARR\s*=\s*9\b", hdr)
    assert (api.FORM_O_APERTURE7, api.FORM_O_SCHARR) == (8, 9)
    assert "hc_canny_device" in api.ABI_SYMBOLS
    assert callable(api.Context.canny_device) and callable(api.Context.canny)
    build.build()
    lib = api.load_library()
    assert lib.hc_canny_device is not None
    assert len(lib.hc_canny_device.argtypes) == 12
    out = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and re.search(r"\bT hc_canny_device\b", out.stdout)
    # a null context is an argument error, before any device is touched
    assert lib.hc_canny_device(None, None, 0, 0, None, 0, 0, 1, 50.0, 150.0, 7, 0) == -1


def _grid():
    vals = [0.0, 0.5, 1.0, 1.5, 7.0, 15.0, 15.5, 15.999, 16.0, 16.001, 16.5, 17.0, 31.999, 32.0, 32.001, 100.0, 150.5, 999.999, 1000.0, 3000.0, 3007.9,
            4000.0, 9000.0, 32766.5, 32767.0, 32767.5, 32768.0, 40000.0, 16 * 32767 - 0.001, 16.0 * 32767, 16 * 32767 + 0.001, 16 * 32767 + 8.0,
            524288.0, 1.0e6, 1.0e9]
    for k in (16 * 3, 16 * 101, 16 * 2047):   # just below / above multiples of 16
        vals += [math.nextafter(k, 0.0), float(k), math.nextafter(k, math.inf), k - 0.25, k + 0.25]
    pairs = [(a, b) for i, a in enumerate(vals) for b in vals[i::5]]
    pairs += [(b, a) for a, b in pairs[::3]]   # swapped
    return [(lo, hi, ap, l2) for lo, hi in pairs for ap in APERTURES for l2 in (0, 1)]


def _run_thresholds(driver, cases, tmp_path):
    path = tmp_path / "cases.txt"
    path.write_text("".join(f"{lo!r} {hi!r} {ap} {l2}\n" if not isinstance(lo, str) else f"{lo} {hi} {ap} {l2}\n" for lo, hi, ap, l2 in cases))
    out = subprocess.run([driver, "thresholds", str(path)], capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases)
    return lines


def test_thresholds_as_canny_cpp(driver, tmp_path):
    cases = _grid()
    assert len(cases) > 2000
    bad = []
    for (lo, hi, ap, l2), line in zip(cases, _run_thresholds(driver, cases, tmp_path)):
        s = 16.0 if ap == 7 else 1.0
        want = X.thresholds(lo / s, hi / s, bool(l2))
        kernel = want if l2 else tuple(min(v, 32767) for v in want)   # the stated clamp of the floored L1 thresholds
        assert max(kernel) <= 32767 * 32767
        if line.split() != [str(v) for v in want + kernel]:
            bad.append(((lo, hi, ap, l2), want, kernel, line))
    assert not bad, f"{len(bad)} of {len(cases)} differ: {bad[:6]}"


def test_clamp_lies_above_every_l1_magnitude():
    """|dx| + |dy| of a u8 source: the two filters' absolute tap sums bound it (aperture 7 after its division by 16)."""
    import deriv_ref as D
    for ap in APERTURES:
        pos = sum(t for t in D.DERIV[ap] if t > 0) * sum(D.SMOOTH[ap]) * 255 >> D.SHIFT[ap]
        assert 2 * pos < 32767 and 2 * pos <= 24480, (ap, pos)


def test_bad_thresholds_and_apertures_refused(driver, tmp_path):
    cases = [("-1", "10", 3, 0), ("10", "-0.001", 7, 1), ("nan", "10", 5, 0), ("10", "nan", -1, 1), ("inf", "10", 3, 0), ("10", "-inf", 7, 0),
             ("-1e300", "-1", 7, 1)]
    cases += [("50", "150", ap, 0) for ap in (0, 1, 4, 9, -3, 2, 6, 8)]
    assert _run_thresholds(driver, cases, tmp_path) == ["refused"] * len(cases)
    assert _run_thresholds(driver, [("0", "0", 7, 1), ("-0.0", "0", 3, 0)], tmp_path) == ["0 0 0 0"] * 2


def test_plans_of_the_new_forms(driver):
    out = subprocess.run([driver, "plans"], capture_output=True, text=True, timeout=900, env=ENV)
    assert out.returncode == 0 and out.stdout.splitlines()[-1].startswith("ok "), out.stdout[-4000:] + out.stderr[-4000:]
    assert int(out.stdout.split()[-1]) > 5000
    plans = [tuple(int(v) for v in l.split()[1:]) for l in out.stdout.splitlines() if l.startswith("plan ")]
    seen = {(ap, ch, piped): form for ap, ch, piped, _, form, *_ in plans}
    assert seen == {(ap, ch, piped): (8 if ap == 7 else 9) for ap in (7, -1) for ch in (1, 3) for piped in (0, 1)}
    # 322 x 97, one frame, two strips: 7 items of 14 rows per strip by the automatic rule (as tests/cpp/plan_driver.cpp pins
    # for aperture 5), hc_set_tuning's rows as they are
    for ap, ch, piped, chunk, form, rows, nchunks, items in plans:
        want_rows = min(chunk, 97) if chunk else 14
        assert (rows, nchunks, items) == (want_rows, -(-97 // want_rows), 2 * -(-97 // want_rows)), (ap, ch, piped, chunk, rows, nchunks, items)
