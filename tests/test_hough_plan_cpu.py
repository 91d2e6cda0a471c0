"""plan_hough_lines, hough_pass, hough_geometry and hough_tables (cudacam_amd/csrc/host_plan.h) without a GPU.
tests/cpp/hough_plan_driver.cpp is compiled against the header with g++ under ASan + UBSan as a stand-alone program, the way
tests/test_blur_plan_cpu.py builds its driver:

* every refusal hc_hough_lines_device documents (null and misaligned pointers, nframes, rho / theta / min_theta / max_theta,
  threshold, an accumulator row beyond LDS, 2^31 cells, sizes that overflow size_t, a scratch bound below one frame); a refused
  plan holds nothing;
* rows per workgroup, groups, frames per pass, passes and scratch at their boundaries (a row that just fits and just does not fit
  LDS; a bound of one frame, one frame minus a byte, k frames); total work = frames x groups; the pointers of every pass;
* the tables of the C++ rule, bit for bit those of tests/hough_ref.py."""
import math
import os
import subprocess

import numpy as np
import pytest

import hough_ref as R
from test_sanitizers import ENV, ROOT, SAN, _cc

DRIVER = os.path.join(ROOT, "tests", "cpp", "hough_plan_driver.cpp")

TABLE_ARGS = [
    (1920, 1080, 1.0, math.pi / 180, 0.0, math.pi),
    (64, 48, 1.0, math.pi / 180, 0.3, 1.2),
    (64, 48, 1.0, math.pi / 4, 0.0, math.pi),
    (64, 48, 1.0, 4.0, 0.0, math.pi),
    (64, 48, 0.5, math.pi / 90, 0.0, math.pi),
    (61, 33, 2.0, math.pi / 180, 0.0, math.pi),
    (61, 33, 3.7, math.pi / 7, 0.0, math.pi),
    (250, 200, 0.3, 0.1, 0.0, math.pi),
    (250, 200, 0.3, 0.01, -1.0, 2.5),
    (7, 5, 3.7, math.pi / 360, 0.7, 0.7),
    (1, 1, 1.0, math.pi / 180, -math.pi, math.pi),
    (640, 480, 1.0 / 3.0, math.pi / 1000, 1e-3, 3.0),
]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hough") / "hough_plan_driver")
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-o", exe, DRIVER])
    return exe


def test_hough_plan_under_asan_ubsan(driver):
    out = subprocess.run([driver], capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-4000:] + out.stderr[-4000:]
    assert int(out.stdout.split()[1]) > 200


@pytest.mark.parametrize("args", TABLE_ARGS)
def test_tables_of_the_cpp_rule_equal_the_restatement(driver, args):
    w, h, rho, theta, lo, hi = args
    out = subprocess.run([driver, "tables", str(w), str(h)] + [float(v).hex() for v in (rho, theta, lo, hi)], capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rows = out.stdout.split("\n")
    numangle, numrho = (int(v) for v in rows[0].split())
    assert (numangle, numrho) == R.geometry(w, h, rho, theta, lo, hi)
    got = np.array([[int(x, 16) for x in r.split()] for r in rows[1:1 + numangle]], np.uint32).reshape(numangle, 3)
    tc, ts, tt = R.tables(w, h, rho, theta, lo, hi)
    for k, want in enumerate((tc, ts, tt)):
        assert np.array_equal(got[:, k], want.view(np.uint32)), ("cos", "sin", "theta")[k]


def test_hough_plan_builds_for_the_legacy_library():
    """host_plan.h keeps compiling without HIP under -DHC_LEGACY_FRONT with the Hough plan in it."""
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", "-DHC_LEGACY_FRONT", "-fsyntax-only", DRIVER])
