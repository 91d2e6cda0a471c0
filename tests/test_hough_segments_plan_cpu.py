"""plan_hough_segments, seg_on_scratch and hough_walk_tables (cudacam_amd/csrc/host_plan.h) without a GPU.
tests/cpp/hough_segments_plan_driver.cpp is compiled against the header with g++ under ASan + UBSan as a stand-alone program, the
way tests/test_hough_plan_cpu.py builds its driver:

* every refusal hc_hough_segments_device documents (null and misaligned pointers, min_length, max_gap, nframes, the view, rho /
  theta / min_theta / max_theta, line_capacity 0, sizes that overflow size_t or a uint32 count); a refused plan holds nothing;
* scratch sizes, grids and scratch pointers at their boundaries;
* the walk tables of the C++ rule, bit for bit those of tests/hough_segments_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import hough_ref as R
import hough_segments_ref as S
from test_hough_plan_cpu import TABLE_ARGS
from test_sanitizers import ENV, ROOT, SAN, _cc

DRIVER = os.path.join(ROOT, "tests", "cpp", "hough_segments_plan_driver.cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hough_segments") / "hough_segments_plan_driver")
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-o", exe, DRIVER])
    return exe


def test_hough_segments_plan_under_asan_ubsan(driver):
    out = subprocess.run([driver], capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-4000:] + out.stderr[-4000:]
    assert int(out.stdout.split()[1]) > 200


@pytest.mark.parametrize("args", TABLE_ARGS)
def test_walk_tables_of_the_cpp_rule_equal_the_restatement(driver, args):
    w, h, rho, theta, lo, hi = args
    out = subprocess.run([driver, "tables", str(w), str(h)] + [float(v).hex() for v in (rho, theta, lo, hi)], capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rows = out.stdout.split("\n")
    numangle = int(rows[0])
    assert numangle == R.geometry(w, h, rho, theta, lo, hi)[0]
    got = [r.split() for r in rows[1:1 + numangle]]
    major, slope, scale = S.walk_tables(w, h, rho, theta, lo, hi)
    assert [int(g[0]) for g in got] == major.tolist()
    assert np.array_equal(np.array([int(g[1], 16) for g in got], np.uint32), slope.view(np.uint32)), "slope"
    assert np.array_equal(np.array([int(g[2], 16) for g in got], np.uint32), scale.view(np.uint32)), "scale"
    assert (np.abs(slope) <= 1).all() and set(major.tolist()) <= {0, 1}


def test_hough_segments_plan_builds_for_the_legacy_library():
    """host_plan.h keeps compiling without HIP under -DHC_LEGACY_FRONT with the segments plan in it."""
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", "-DHC_LEGACY_FRONT", "-fsyntax-only", DRIVER])
