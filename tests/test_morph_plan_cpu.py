"""plan_morphology, morph_pass and structuring_spans (cudacam_amd/csrc/host_plan.h) without a GPU.
tests/cpp/morph_plan_driver.cpp is compiled against the header with g++ under ASan + UBSan, the way tests/test_blur_plan_cpu.py
builds its driver:

* item counts at strip and chunk boundaries, total_items = n x strips x chunks; 1080p x 512 maps pinned by hand;
* in_aligned / out_aligned by the low bits of address, pitch and frame stride of each side; the views by value;
* the levels of an element (its distinct half-widths, ascending) and the level of every row; the three pinned tables of
  structuring_spans, whose refusals write nothing;
* every refusal hc_morphology_device documents: null pointers, channels outside {1, 3} or 3 on a one-channel context, an op
  outside the enum, ksize outside {3, 5, 7}, a span outside -1 .. K/2 in every row, all rows empty, pitches smaller than a row
  of the CALLER's channels, nframes < 1 and above the limit by channels / per_channel, a frame stride below height * pitch at
  n = 2, height * pitch >= 2^32 on either side, a view that wraps the address space, overlapping views (in place, one shared
  byte on either side); views that touch pass; a refused plan holds nothing to launch;
* the launches of each operation (complement / subtract, the scratch between the stages of OPEN / CLOSE at a pitch of whole
  dwords) and the passes at scratch bounds of exactly k frames, one byte less, and below one frame (refused)."""
import os
import subprocess

from test_sanitizers import ENV, ROOT, SAN, _cc

DRIVER = os.path.join(ROOT, "tests", "cpp", "morph_plan_driver.cpp")


def test_morph_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "morph_plan_driver")
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-o", exe, DRIVER])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-4000:] + out.stderr[-4000:]
    assert int(out.stdout.split()[1]) > 100000


def test_morph_plan_builds_for_the_legacy_library():
    """host_plan.h keeps compiling without HIP under -DHC_LEGACY_FRONT with the morphology plan in it."""
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", "-DHC_LEGACY_FRONT", "-fsyntax-only", DRIVER])
