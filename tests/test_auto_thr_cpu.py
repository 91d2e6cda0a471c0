"""Per-frame and automatic thresholds of Mode O without a GPU.

* include/hipcanny.h, api.py and the built library agree on hc_frame_thresholds_device, hc_histogram_device and
  hc_auto_thresholds_device: signatures, exported symbols, and a null context is HC_E_ARG before any device is touched.
* cudacam_amd/csrc/auto_thr.h, compiled with g++ under ASan + UBSan into tests/cpp/auto_thr_driver.cpp, equals the numpy
  restatement tests/auto_thr_ref.py on the histograms of flat frames of every grey level, two-level frames at every split of
  N = 6 and N = 7 samples, 200 seeded random histograms with up to 2^27 samples and the synth natural / noise / steps frames at
  64 x 48 -- each with sigma in {0, 0.33, 1} and ratio in {0, 0.5, 1} -- plus worked answers stated here.
* frame_threshold_pair (canny_params.h: what the kernels make of a table entry) equals hc_set_thresholds followed by
  plan_thresholds_and_masks on a grid of pairs with negatives, values above 32767, swapped pairs and both L2 settings.
* the planner: no plan carries a table, and the plans of the driver's sweep are field for field those of the commit named
  in tests/golden/auto_thr_plans.json (its digest was recorded with this driver compiled against that commit's planner)."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import auto_thr_ref as R
from cudacam_amd import api, build, synth
from test_sanitizers import ENV, ROOT, SAN, _cc

DRIVER = os.path.join(ROOT, "tests", "cpp", "auto_thr_driver.cpp")
SIGMAS = (0.0, 0.33, 1.0)
RATIOS = (0.0, 0.5, 1.0)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("auto_thr") / "auto_thr_driver")
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *SAN, "-o", exe, DRIVER])
    return exe


def _args(hdr, name):
    m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
    assert m, f"include/hipcanny.h does not declare {name}"
    body = re.sub(r"/\*.*?\*/", " ", m.group(1).replace("\n", " "))
    return [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*").strip() for a in body.split(",")]


def test_header_api_and_library_agree():
    hdr = open(os.path.join(ROOT, "include", "hipcanny.h")).read()
    assert _args(hdr, "hc_frame_thresholds_device") == ["hc_ctx*", "const void*", "int"]
    assert _args(hdr, "hc_histogram_device") == ["hc_ctx*", "const void*", "size_t", "size_t", "int", "void*"]
    assert _args(hdr, "hc_auto_thresholds_device") == ["hc_ctx*", "const void*", "size_t", "size_t", "int", "int", "double", "void*"]
    assert re.search(r"\bHC_AUTO_MEDIAN\s*=\s*0\b", hdr) and re.search(r"\bHC_AUTO_OTSU\s*=\s*1\b", hdr)
    assert (api.AUTO_MEDIAN, api.AUTO_OTSU) == (0, 1) == (R.MEDIAN, R.OTSU)
    for name in ("hc_frame_thresholds_device", "hc_histogram_device", "hc_auto_thresholds_device"):
        assert name in api.ABI_SYMBOLS
    for meth in ("frame_thresholds_device", "histogram_device", "auto_thresholds_device", "histogram", "canny_auto"):
        assert callable(getattr(api.Context, meth))
    build.build()
    lib = api.load_library()
    assert [len(getattr(lib, n).argtypes) for n in ("hc_frame_thresholds_device", "hc_histogram_device", "hc_auto_thresholds_device")] == [3, 6, 8]
    out = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0
    for name in ("hc_frame_thresholds_device", "hc_histogram_device", "hc_auto_thresholds_device"):
        assert re.search(r"\bT %s\b" % name, out.stdout), name
    # the two kernels of stats.hip are in the product library
    blob = open(api.LIB_PATH, "rb").read()
    assert b"k_hist256" in blob and b"k_auto_thr" in blob
    # a null context is an argument error, before any device is touched
    assert lib.hc_frame_thresholds_device(None, None, 1) == -1
    assert lib.hc_histogram_device(None, None, 0, 0, 1, None) == -1
    assert lib.hc_auto_thresholds_device(None, None, 0, 0, 1, 0, 0.33, None) == -1


def test_canny_auto_queues_without_a_host_sync():
    """auto thresholds -> table -> run are queued back to back: nothing synchronises between the first and the last."""
    import inspect
    src = inspect.getsource(api.Context.canny_auto)
    a, b, c = (src.index(s) for s in ("self.auto_thresholds_device(", "self.frame_thresholds_device(thr", "self.run_device("))
    assert a < b < c
    between = src[a:src.index("\n", c)]
    assert "sync" not in between and ".cpu()" not in between and ".item()" not in between


# ---- the rules ---------------------------------------------------------------------------------------------------------
def _hist_of(values_counts):
    h = np.zeros(256, np.int64)
    for v, c in values_counts:
        h[v] += c
    return h


def _cases():
    hists = []
    for v in range(256):                                   # flat frames of every grey level
        hists.append(_hist_of([(v, 64 * 48)]))
    rng = np.random.default_rng(20261019)
    for n in (6, 7):                                       # two-level frames at every split (even and odd counts, a != b)
        for k in range(1, n):
            for lo, hi in ((0, 255), (10, 11), (100, 200), (254, 255), (0, 1)):
                hists.append(_hist_of([(lo, k), (hi, n - k)]))
    for i in range(200):                                   # random histograms, up to 2^27 samples
        total = int(rng.integers(1, (1 << 27) + 1)) if i % 4 else (1 << 27)
        nb = int(rng.integers(1, 257))
        bins = rng.choice(256, size=nb, replace=False)
        w = rng.random(nb) ** int(rng.integers(1, 6))
        cnt = np.floor(w / w.sum() * total).astype(np.int64)
        cnt[0] += total - int(cnt.sum())
        h = np.zeros(256, np.int64)
        h[bins] = cnt
        assert int(h.sum()) == total and h.min() >= 0
        hists.append(h)
    for f in (synth.natural(64, 48, 3), synth.noise(64, 48, 4), synth.steps(64, 48, 200, "vertical"), synth.steps(64, 48, 90, "diagonal", base=20)):
        hists.append(R.histogram(f))
    return hists


def _run_hist(driver, rows, tmp_path):
    path = tmp_path / "hists.txt"
    path.write_text("".join(f"{rule} {param!r} " + " ".join(str(int(c)) for c in h) + "\n" for rule, param, h in rows))
    out = subprocess.run([driver, "hist", str(path)], capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(rows)
    return lines


def test_header_equals_the_restatement(driver, tmp_path):
    hists = _cases()
    assert len(hists) == 256 + 55 + 200 + 4
    rows = [(R.MEDIAN, s, h) for h in hists for s in SIGMAS] + [(R.OTSU, r, h) for h in hists for r in RATIOS]
    bad = []
    for (rule, param, h), line in zip(rows, _run_hist(driver, rows, tmp_path)):
        want = R.from_histogram(h, rule, param)
        if line.split() != [str(v) for v in want]:
            bad.append((rule, param, np.flatnonzero(h)[:6].tolist(), want, line))
    assert not bad, f"{len(bad)} of {len(rows)} differ: {bad[:6]}"


def test_restatement_from_frames_is_the_histogram_form():
    for f in (synth.natural(64, 48, 3), synth.noise(64, 48, 4), np.stack([synth.natural(64, 48, 5), synth.noise(64, 48, 6), synth.flat(64, 48, 9)], -1)):
        for rule, params in ((R.MEDIAN, SIGMAS), (R.OTSU, RATIOS)):
            for p in params:
                assert R.thresholds(f, rule, p) == R.from_histogram(R.histogram(f), rule, p)


def test_worked_answers(driver, tmp_path):
    n = 64 * 48
    rows, want = [], []

    def add(rule, param, h, pair):
        rows.append((rule, param, h))
        want.append(pair)

    # a flat frame of grey level v: the median is v; no threshold splits the samples, Otsu's t* = 0
    add(R.MEDIAN, 0.33, _hist_of([(100, n)]), (67, 133))      # int(0.67 * 100.0) = 67 (67.00000000000001), int(1.33 * 100.0) = 133
    add(R.MEDIAN, 0.0, _hist_of([(100, n)]), (100, 100))
    add(R.MEDIAN, 1.0, _hist_of([(200, n)]), (0, 255))        # 2 * 200 capped at 255
    add(R.MEDIAN, 0.33, _hist_of([(0, n)]), (0, 0))
    add(R.OTSU, 0.5, _hist_of([(100, n)]), (0, 0))
    add(R.OTSU, 1.0, _hist_of([(255, n)]), (0, 0))
    # half 0 / half 255, even N: a = 0, b = 255, v = 127.5
    add(R.MEDIAN, 0.0, _hist_of([(0, n // 2), (255, n // 2)]), (127, 127))
    add(R.MEDIAN, 0.33, _hist_of([(0, n // 2), (255, n // 2)]), (85, 169))   # 0.67 * 127.5 = 85.425, 1.33 * 127.5 = 169.575
    add(R.MEDIAN, 1.0, _hist_of([(0, n // 2), (255, n // 2)]), (0, 255))
    # ... odd N with one more 255: both middle samples are 255
    add(R.MEDIAN, 0.0, _hist_of([(0, 3), (255, 4)]), (255, 255))
    # two levels 0 / 255: every t in 0..254 splits them alike, the smallest wins: t* = 0
    add(R.OTSU, 0.5, _hist_of([(0, n // 2), (255, n // 2)]), (0, 0))
    # two levels 100 / 200: the score is the same for t = 100 .. 199 and smaller elsewhere: t* = 100
    add(R.OTSU, 0.5, _hist_of([(100, 5), (200, 7)]), (50, 100))
    add(R.OTSU, 1.0, _hist_of([(100, 5), (200, 7)]), (100, 100))
    add(R.OTSU, 0.0, _hist_of([(100, 5), (200, 7)]), (0, 100))
    # three levels 10 x 4, 20 x 4, 200 x 1: N = 9, S = 320; t = 10: d = 320 * 4 - 9 * 40 = 920, 920^2 / (4 * 5) = 42320;
    # t = 20: d = 320 * 8 - 9 * 120 = 1480, 1480^2 / (8 * 1) = 273800: t* = 20
    add(R.OTSU, 0.5, _hist_of([(10, 4), (20, 4), (200, 1)]), (10, 20))
    assert float(np.median(np.array([0] * 4 + [255] * 4, np.uint8))) == 127.5
    got = _run_hist(driver, rows, tmp_path)
    for (rule, param, h), pair, line in zip(rows, want, got):
        assert R.from_histogram(h, rule, param) == pair, (rule, param, pair)
        assert line.split() == [str(v) for v in pair], (rule, param, pair, line)


def test_bad_rules_and_params_refused(driver, tmp_path):
    h = _hist_of([(5, 10)])
    rows = [(2, 0.5, h), (-1, 0.5, h), (0, -0.001, h), (0, 1.001, h), (1, 2.0, h), (1, float("nan"), h), (0, float("inf"), h), (1, float("-inf"), h)]
    assert _run_hist(driver, rows, tmp_path) == ["refused"] * len(rows)


# ---- the per-frame pair ------------------------------------------------------------------------------------------------
def test_frame_threshold_pair_is_set_thresholds_and_the_plan(driver, tmp_path):
    vals = [-(1 << 31), -70000, -32768, -1, 0, 1, 2, 50, 150, 255, 2040, 24480, 32766, 32767, 32768, 65535, 70000, (1 << 31) - 1]
    cases = [(lo, hi, l2) for lo in vals for hi in vals for l2 in (0, 1)]
    assert any(lo > hi for lo, hi, _ in cases) and any(lo < 0 for lo, _, _ in cases) and any(hi > 32767 for _, hi, _ in cases)
    path = tmp_path / "pairs.txt"
    path.write_text("".join(f"{lo} {hi} {l2}\n" for lo, hi, l2 in cases))
    out = subprocess.run([driver, "pairs", str(path)], capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases)
    for (lo, hi, l2), line in zip(cases, lines):
        a_lo, a_hi, p_lo, p_hi = (int(v) for v in line.split())
        n_lo, n_hi = R.normalised(lo, hi)
        want = (n_lo * n_lo, n_hi * n_hi) if l2 else (n_lo, n_hi)
        assert (a_lo, a_hi) == (p_lo, p_hi) == want, (lo, hi, l2, line, want)


# ---- the planner -------------------------------------------------------------------------------------------------------
def test_plans_are_those_of_the_parent_and_carry_no_table(driver):
    with open(os.path.join(ROOT, "tests", "golden", "auto_thr_plans.json")) as f:
        golden = json.load(f)
    out = subprocess.run([driver, "plans"], capture_output=True, text=True, timeout=900, env=ENV)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-4000:] + out.stderr[-4000:]
    words = out.stdout.split()
    assert (int(words[1]), words[2]) == (golden["plans"], golden["digest"])
    assert int(words[1]) > 100000
