"""plan_distance_transform (cudacam_amd/csrc/host_plan.h) without a GPU.  tests/cpp/dist_plan_driver.cpp is compiled against the
header with g++ under ASan + UBSan, the way tests/test_morph_plan_cpu.py builds its driver:

* the grids of k_dt_cols at the wave boundaries (63, 64, 65 ... 16384 columns) and of k_dt_rows at the row-group boundaries, the
  bytes of its LDS row, for every width up to 600;
* every refusal hc_distance_transform_device documents, by its message: null pointers, a target or dist_type outside its enum,
  pitches smaller than a row, output bases, pitches and strides that are no multiple of 4, height * pitch >= 2^32 on each of the
  three sides, nframes outside 1 .. max_frames, a frame stride below height * pitch at n = 2, views that wrap the address space,
  W * H >= 2^31 - 1, (W - 1)^2 + (H - 1)^2 >= 2^31 - 1 at its exact edge, W = 16385 (16384 passes with 64 KiB);
* every pair of views overlapping by one word in both orders; views that touch pass; the two outputs as ROIs of one plane side by
  side pass, and are refused once they share a word, run into the next row or differ in pitch or frame stride;
* a refused plan holds nothing to launch; a call without a nearest plane does not look at its pitch and stride."""
import os
import subprocess

from test_sanitizers import ENV, ROOT, SAN, _cc

DRIVER = os.path.join(ROOT, "tests", "cpp", "dist_plan_driver.cpp")


def test_dist_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "dist_plan_driver")
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-o", exe, DRIVER])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-4000:] + out.stderr[-4000:]
    assert int(out.stdout.split()[1]) > 4000


def test_dist_plan_builds_for_the_legacy_library():
    """host_plan.h keeps compiling without HIP under -DHC_LEGACY_FRONT with the distance transform's plan in it."""
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", "-DHC_LEGACY_FRONT", "-fsyntax-only", DRIVER])
