"""plan_pyr_down and plan_lk_flow (cudacam_amd/csrc/host_plan.h) without a GPU.
tests/cpp/flow_plan_driver.cpp is compiled against the header with g++ under ASan + UBSan as a stand-alone program, the way
tests/test_corner_plan_cpu.py builds its driver:

* the level geometry of k_pyr_down8 -- destination sizes, strips and row chunks at source sizes around their seams, the alignment
  flags of both sides by the low bits of address, pitch and frame stride, the parameter block by value; 1080p x 64 pinned by hand;
* the launch grid and the round classes of k_lk_flow for every window, eps2 and min_eig as the kernel receives them;
* every refusal hc_pyr_down_device and hc_lk_flow_device document, one by one, each beside its nearest neighbour that passes; a
  refused plan holds nothing to launch."""
import os
import subprocess

from test_sanitizers import ENV, ROOT, SAN, _cc

DRIVER = os.path.join(ROOT, "tests", "cpp", "flow_plan_driver.cpp")


def test_flow_plans_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "flow_plan_driver")
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-o", exe, DRIVER])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-4000:] + out.stderr[-4000:]
    assert int(out.stdout.split()[1]) > 1000


def test_flow_plans_build_for_the_legacy_library():
    """host_plan.h keeps compiling without HIP under -DHC_LEGACY_FRONT with the flow plans in it."""
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", "-DHC_LEGACY_FRONT", "-fsyntax-only", DRIVER])
