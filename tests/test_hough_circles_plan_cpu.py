"""plan_hough_circles, circle_pass and hough_circle_geometry (cudacam_amd/csrc/host_plan.h) without a GPU.
tests/cpp/hough_circles_plan_driver.cpp is compiled against the header with g++ under ASan + UBSan as a stand-alone program, the
way tests/test_hough_plan_cpu.py builds its driver:

* every refusal hc_hough_circles_device documents, by its message; a refused plan holds nothing;
* scratch bytes, frames per pass, passes, the grids the launch reads and the scratch sections of every pass, under the default bound and small ones;
* the guards at 2^20 (width / height + max_radius) and 2^31 (accumulator cells);
* the geometry of the C++ rule against tests/hough_circles_ref.py over a sweep of sizes, dp and min_dist."""
import os
import subprocess

import pytest

import hough_circles_ref as HC
from test_sanitizers import ENV, ROOT, SAN, _cc

DRIVER = os.path.join(ROOT, "tests", "cpp", "hough_circles_plan_driver.cpp")

SIZES = [(1, 1), (9, 7), (33, 31), (64, 48), (65, 64), (130, 67), (200, 150), (640, 480), (1920, 1080), (3840, 2160), (1000003, 3)]
DPS = [1.0, 1.5, 2.0, 1.25, 3.0, 7.3, 100.0, 1e6]
MIN_DISTS = [0.0, 1.0, 2.5, 3.0, 17.25, 1e3, 1e200]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("circles") / "hough_circles_plan_driver")
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-o", exe, DRIVER])
    return exe


def test_circle_plan_under_asan_ubsan(driver):
    out = subprocess.run([driver], capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-4000:] + out.stderr[-4000:]
    assert int(out.stdout.split()[1]) > 1000


def _geometry(driver, w, h, dp, min_dist, rmin, rmax):
    return subprocess.run([driver, "geometry", str(w), str(h), float(dp).hex(), float(min_dist).hex(), str(rmin), str(rmax)], capture_output=True, text=True, timeout=600, env=ENV)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_geometry_of_the_cpp_rule_equals_the_restatement(driver, size):
    w, h = size
    for dp in DPS:
        for md in MIN_DISTS:
            out = _geometry(driver, w, h, dp, md * dp, 3, 40)
            assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
            assert tuple(int(v) for v in out.stdout.split()) == HC.geometry(w, h, dp, md * dp, 3, 40), (dp, md)


def test_geometry_refusals_agree_with_the_restatement(driver):
    for args in ((0, 5, 1.0, 0, 1, 2), (5, 5, 0.99, 0, 1, 2), (5, 5, float("nan"), 0, 1, 2), (5, 5, 1.0, -1.0, 1, 2), (5, 5, 1.0, float("inf"), 1, 2), (5, 5, 1.0, 0, 0, 2),
                 (5, 5, 1.0, 0, 3, 2), (5, 5, 1.0, 0, 1, 4095), (5, 5, 1.0, 0, (1 << 20) - 8, (1 << 20) - 5), (5, 5, 1e300, 0, 1, 2)):
        out = _geometry(driver, *args)
        assert out.returncode == 1 and out.stdout.startswith("refused: "), (args, out.stdout, out.stderr[-2000:])
        with pytest.raises(ValueError):
            HC.geometry(*args)


def test_circle_plan_builds_for_the_legacy_library():
    """host_plan.h keeps compiling without HIP under -DHC_LEGACY_FRONT with the circle plan in it."""
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", "-DHC_LEGACY_FRONT", "-fsyntax-only", DRIVER])
