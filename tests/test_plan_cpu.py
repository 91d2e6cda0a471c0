"""The host planner (cudacam_amd/csrc/host_plan.h: plan_front, plan_hyst, HystHistory, ChainWatch, pipeline_slots) without
a GPU.  tests/cpp/plan_driver.cpp is compiled against the header with g++ under ASan + UBSan and sweeps every width
1..8184 at heights 1 / 8 / 480 / 1080 / 4320 and every height 1..4400 at widths 1 / 8 / 240 / 248 / 496 / 640 / 1920 /
3840 / 8184 (both modes, 1 and 3 channels, per-channel, plain and pipelined, batches up to the first one the 0.5 G-pixel
slot rule calls big), and the whole option product where width and height are both of 1, 7, 8, 16, 240 / 248 / 496 +- 1,
480, 1079, 1080, 2160, 4320.  Every plan must keep what the launchers and kernels rest on:

* nchunks * run_rows >= H; total_items = units x chunks > 0 for each form; rows of the 8-px forms hold whole groups;
* the 4-px Mode O forms (-1, 6, 7) take hc_set_tuning's rows per work item as they are, chunk_rows = min(max(chunk, 1), H)
  (1, 7, 17 among the swept values); their automatic split pinned for one frame and for one and two items per strip;
* the runs hc_set_tuning's length gives the 8-px forms (2, 4, 3, 5) on the shapes of tests/test_gpu_front8_runs.py: rows per
  run, runs per strip and items pinned for every run length 6 k - 4 of 41 rows, the heights that give each last-run length,
  each form once, and both sides of k_front_mx's block borders (12 | 13, 28 | 29);
* a HALF plan satisfies the `fits` inequalities; a plan with the provisional map never has H * pitch >= 2^32;
* wl_stride <= wl_cap; zeroed_words and FLAG_WORDS + WL_COUNT_WORDS + 2 * wl_stride within the d_flags allocation;
* 1 <= K <= MAX_HYST_LAUNCHES; the loop form only for <= HYST_LOOP_MAX_TILES tiles of the two whitelisted shapes;
  per-launch list modes 0 .. 0, 2, 1 .. 1 when mixed;
* the forms the GPU tests pin (half strips, k_front_mx, k_front_o_ext, the 4 GiB views, the smoke run);
* ChainWatch on synthetic traces: trial after three outlasting runs and run >= 5, kept only below 0.97 x the pre-trial
  mean, back-off 64 doubling to 4096, back to two slots after 16 light runs doubling to 1024, one wave above 0.25 and
  back below 0.03, the chain_told overrides;
* check_view on each entry point's view specification (row bytes, alignment, 4 GiB rule): tight and padded views pass,
  each single defect is its own rule (pitch = row - 1; stride = pitch * H - 1 at n = 2, accepted at n = 1; odd address,
  pitch, stride of int16 views; both sides of H * pitch = 2^32, pitch 1 << 31 and (1 << 32) / H), and pitches from
  2^64 / H to SIZE_MAX, whose H * pitch wraps 64 bits, are refused with UBSan silent;
* plan_derivatives, plan_histogram, plan_edge_points over W 1..600 x H 1..300, C 1 / 3, n 1 / 2 / max_batch: the chunks
  cover H with no empty one, total_items = n x strips x chunks, out_align and in_aligned by the low bits, the edge-item
  table holds every batch; 64 x 32 x 3 (n 2), 1920 x 1080 (n 1024) and 1 x 1 pinned by hand; the refusals.
  (Neither counted as plans nor folded into the digest.)

The driver also folds every field of every front plan it makes into a 64-bit FNV-1a digest.  tests/golden/
plan_front_digest.json holds the plan count and the digests of both builds (the product's, and -DHC_LEGACY_FRONT) as the
planner of the commit named there gave them: a planner that is restructured must still plan exactly that.  The legacy
digest leaves out two values no kernel reads (`subchunks` but for form 0, `run_rows` of forms -1 / 6 / 7)."""
import json
import os
import subprocess

from test_sanitizers import ENV, ROOT, SAN, _cc


DRIVER = os.path.join(ROOT, "tests", "cpp", "plan_driver.cpp")
with open(os.path.join(ROOT, "tests", "golden", "plan_front_digest.json")) as _f:
    GOLDEN = json.load(_f)


def _run_driver(exe, env=None):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=1500, env=env)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-4000:] + out.stderr[-4000:]
    return out.stdout.split()


def test_planner_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "plan_driver")
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-o", exe, DRIVER])
    words = _run_driver(exe, ENV)
    assert int(words[1]) > 10 * 1000 * 1000
    assert (int(words[1]), words[2]) == (GOLDEN["plans"], GOLDEN["digest"])


def test_planner_builds_for_the_legacy_library(tmp_path):
    """The round-1 arithmetic (HC_LEGACY_FRONT) stays behind its macro and compiles without HIP as well."""
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", "-DHC_LEGACY_FRONT", "-fsyntax-only", DRIVER])


def test_legacy_planner_plans_what_the_golden_commit_planned(tmp_path):
    """The -DHC_LEGACY_FRONT build run as well (-O2, no sanitizers): its invariants, pinned plans and digest."""
    exe = str(tmp_path / "plan_driver_legacy")
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", "-O2", "-DHC_LEGACY_FRONT", "-o", exe, DRIVER])
    words = _run_driver(exe)
    assert (int(words[1]), words[2]) == (GOLDEN["plans"], GOLDEN["digest_legacy"])
