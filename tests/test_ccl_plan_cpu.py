"""plan_connected_components and ccl_pass (cudacam_amd/csrc/host_plan.h) without a GPU.  tests/cpp/ccl_plan_driver.cpp is compiled
against the header with g++ under ASan + UBSan as a stand-alone program, the way tests/test_hough_circles_plan_cpu.py builds its
driver:

* every refusal hc_connected_components_device documents, by its message; a refused plan holds nothing;
* tiles, border pixels, row chunks, row groups, passes and scratch bytes under the default bound and small ones, and the views and
  rows of every pass;
* the guards at 2^31 - 1 pixels and at 2^32 row bytes of either view."""
import os
import subprocess

import pytest

from test_sanitizers import ENV, ROOT, SAN, _cc

DRIVER = os.path.join(ROOT, "tests", "cpp", "ccl_plan_driver.cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ccl") / "ccl_plan_driver")
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-o", exe, DRIVER])
    return exe


def test_ccl_plan_under_asan_ubsan(driver):
    out = subprocess.run([driver], capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-4000:] + out.stderr[-4000:]
    assert int(out.stdout.split()[1]) > 150


def test_ccl_plan_builds_for_the_legacy_library():
    """host_plan.h keeps compiling without HIP under -DHC_LEGACY_FRONT with the component plan in it."""
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", "-DHC_LEGACY_FRONT", "-fsyntax-only", DRIVER])
