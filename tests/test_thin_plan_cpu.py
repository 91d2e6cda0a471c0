"""plan_thinning and thin_pass (cudacam_amd/csrc/host_plan.h) without a GPU.
tests/cpp/thin_plan_driver.cpp is compiled against the header with g++ under ASan + UBSan as a stand-alone program, the way
tests/test_morph_plan_cpu.py builds its driver:

* words per row and panels at W = 1, 31, 32, 33, 2047, 2048, 2049, 8184, tiles at heights around the rows per tile, the bytes of a
  plane, a table and a frame of scratch, in_aligned / out_aligned by the low bits of address, pitch and frame stride of each side,
  the three parameter blocks by value; 1080p x 64 maps pinned by hand;
* every refusal hc_thinning_device documents, one by one, each beside a neighbour that passes: null views (a null d_status is
  fine), a method outside the enum, max_iterations 0 and 1025 (1 and 1024 pass), a d_status that is not 4-byte aligned, a pitch
  below a row on either side (an odd-aligned view passes), height * pitch >= 2^32, nframes outside 1 .. max_batch (3 * max_batch
  on a per-channel context), a frame stride below height * pitch at n = 2, a view that wraps the address space, overlapping views
  (in place, one shared byte on either side; views that touch pass), one frame's scratch above the bound; a refused plan holds
  nothing to launch;
* the bit-sliced decision of k_thin_step (thin_removed, canny_params.h: the text the kernel compiles) for all 256 neighbourhoods
  with and without the centre pixel, alone at every bit position and 32 side by side in a word, both methods and
  sub-iterations, against the header's rules written out per pixel;
* the passes under lowered bounds: frames per pass at bounds of exactly k frames and one byte less, the short last pass, the
  offsets of pass k into both views, the status table and the scratch."""
import os
import subprocess

from test_sanitizers import ENV, ROOT, SAN, _cc

DRIVER = os.path.join(ROOT, "tests", "cpp", "thin_plan_driver.cpp")


def test_thin_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "thin_plan_driver")
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-o", exe, DRIVER])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-4000:] + out.stderr[-4000:]
    assert int(out.stdout.split()[1]) > 100000


def test_thin_plan_builds_for_the_legacy_library():
    """host_plan.h keeps compiling without HIP under -DHC_LEGACY_FRONT with the thinning plan in it."""
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", "-DHC_LEGACY_FRONT", "-fsyntax-only", DRIVER])
