"""plan_gaussian_blur, border_index and gaussian_taps_q8 (cudacam_amd/csrc/host_plan.h, canny_params.h) without a GPU.
tests/cpp/blur_plan_driver.cpp is compiled against the header with g++ under ASan + UBSan, the way tests/test_plan_cpu.py
builds plan_driver.cpp:

* item counts at strip and chunk boundaries (W = strip - 1, strip, strip + 1, ...; H = chunk - 1, chunk, chunk + 1, ...),
  total_items = n x strips x chunks; 1080p x 512 frames pinned by hand;
* in_aligned / out_aligned by the low bits of address, pitch and frame stride of each side; the views and the taps by value;
* every refusal hc_gaussian_blur_device documents except nframes > max_batch (check_views' own rule): null pointers, ksize
  outside {3, 5, 7}, a border outside the enum, a tap above 256, tap sums of 255, 257 and 0, pitches smaller than a row,
  nframes < 1, a frame stride below height * pitch at n = 2, height * pitch >= 2^32 on either side, views that wrap the
  address space, overlapping views (in place, one shared byte on either side, the last frame of a batch, interleaved ROIs);
  views that touch pass; a refused plan holds nothing to launch;
* border_index against a walk along the axis for lengths 1..12 and indices -30..41, both borders;
* gaussian_taps_q8: the fixed tables, symmetric sets of sum 256 that the plan accepts for sigma 1e-300 .. 1e300, and
  refusals that write nothing."""
import os
import subprocess

from test_sanitizers import ENV, ROOT, SAN, _cc

DRIVER = os.path.join(ROOT, "tests", "cpp", "blur_plan_driver.cpp")


def test_blur_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "blur_plan_driver")
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-o", exe, DRIVER])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-4000:] + out.stderr[-4000:]
    assert int(out.stdout.split()[1]) > 100000


def test_blur_plan_builds_for_the_legacy_library():
    """host_plan.h keeps compiling without HIP under -DHC_LEGACY_FRONT with the blur plan in it."""
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", "-DHC_LEGACY_FRONT", "-fsyntax-only", DRIVER])
