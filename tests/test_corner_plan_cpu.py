"""plan_corner_response, plan_good_features and feat_pass (cudacam_amd/csrc/host_plan.h) without a GPU.
tests/cpp/corner_plan_driver.cpp is compiled against the header with g++ under ASan + UBSan as a stand-alone program, the way
tests/test_thin_plan_cpu.py builds its driver:

* strips and row chunks of k_corner_response at widths and heights around their seams, the alignment classes of both sides by the
  low bits of address, pitch and frame stride, the parameter block by value; 1080p x 64 frames pinned by hand;
* every refusal hc_corner_response_device and hc_good_features_device document, one by one, each beside its nearest neighbour that
  passes; a refused plan holds nothing to launch;
* min_d2 at 0, 1, sqrt 2, 1e9 and the 2^62 cap, and that it is the smallest such integer;
* the passes under lowered scratch bounds: frames per pass at bounds of exactly k frames and one byte less, the short last pass,
  the offsets of pass k into the view, the outputs and the scratch, the range a pass zeroes;
* the key / digit helpers of the radix select (canny_params.h: the text the kernels compile) -- keys of special values, digits
  that rebuild the key -- and the cut they find from the top digit down against the sorted list, on lists of few distinct keys that
  differ inside one digit or across a digit boundary.  (The histogram walk itself is a wave-parallel scan in the kernel, not plain
  C++ shared with the host; the driver walks the same histograms serially.)"""
import os
import subprocess

from test_sanitizers import ENV, ROOT, SAN, _cc

DRIVER = os.path.join(ROOT, "tests", "cpp", "corner_plan_driver.cpp")


def test_corner_plans_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "corner_plan_driver")
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-o", exe, DRIVER])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-4000:] + out.stderr[-4000:]
    assert int(out.stdout.split()[1]) > 20000


def test_corner_plans_build_for_the_legacy_library():
    """host_plan.h keeps compiling without HIP under -DHC_LEGACY_FRONT with the corner plans in it."""
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", "-DHC_LEGACY_FRONT", "-fsyntax-only", DRIVER])
