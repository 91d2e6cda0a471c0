"""tests/dist_ref.py, the restatement the GPU tests of hc_distance_transform_device compare with, and the entry's C ABI, without
a GPU: hand-made known answers (the tie rules among them); the brute-force and the separable restatement against each other on a
few hundred random frames; the distances against scipy.ndimage.distance_transform_edt (its indices break ties differently, so
only the distances are anchored there); the float32 rule of HC_DT_F32 around and above 2^24; the header's prototype and constants
against api.py, the symbol in both libraries and the test library's refusal."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import dist_ref as R
from cudacam_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "hc_distance_transform_device"
ARGS = (None, 16, 64, 64 * 48, 1, 0, 0, 4096, 256, 256 * 48, 8192, 256, 256 * 48)


def _both(m, target=R.TO_NONZERO):
    a, b, c = R.brute_force(m, target), R.separable(m, target), R.vectorised(m, target)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]) and c[0].dtype == c[1].dtype == np.int32
    return a


def test_a_single_pixel():
    m = np.zeros((5, 7), np.uint8)
    m[3, 2] = 255
    d2, near = _both(m)
    yy, xx = np.mgrid[0:5, 0:7]
    assert np.array_equal(d2, (xx - 2) ** 2 + (yy - 3) ** 2) and (near == 3 * 7 + 2).all()
    assert d2.dtype == np.int32 and near.dtype == np.int32


def test_a_full_row():
    m = np.zeros((6, 9), np.uint8)
    m[4] = 1
    d2, near = _both(m)
    yy, xx = np.mgrid[0:6, 0:9]
    assert np.array_equal(d2, (yy - 4) ** 2) and np.array_equal(near, 4 * 9 + xx)


def test_a_tie_along_the_row_goes_to_the_smaller_x():
    m = np.zeros((1, 5), np.uint8)
    m[0, 0] = m[0, 4] = 255
    d2, near = _both(m)
    assert d2[0].tolist() == [0, 1, 4, 1, 0] and near[0].tolist() == [0, 0, 0, 4, 4]


def test_a_3_4_5_tie_against_a_straight_5():
    # query (5, 0): (0, 0) straight left at 5, (2, 4) and (8, 4) at 3-4-5: all at d2 = 25 -> the smallest x' is (0, 0)
    m = np.zeros((5, 11), np.uint8)
    m[0, 0] = m[4, 2] = m[4, 8] = 255
    d2, near = _both(m)
    assert d2[0, 5] == 25 and near[0, 5] == 0
    m[0, 0] = 0   # without it: (2, 4) before (8, 4)
    d2, near = _both(m)
    assert d2[0, 5] == 25 and near[0, 5] == 4 * 11 + 2
    # a straight 5 on the RIGHT against a 3-4-5 on the left: the left one has the smaller x'
    m = np.zeros((5, 11), np.uint8)
    m[0, 10] = m[4, 2] = 255
    d2, near = _both(m)
    assert d2[0, 5] == 25 and near[0, 5] == 4 * 11 + 2


def test_a_tie_between_above_and_below_goes_to_the_one_above():
    m = np.zeros((5, 3), np.uint8)
    m[0, 1] = m[4, 1] = 255
    d2, near = _both(m)
    assert d2[2].tolist() == [5, 4, 5] and near[2].tolist() == [1, 1, 1]
    assert near[3].tolist() == [13, 13, 13] and near[1].tolist() == [1, 1, 1]


def test_an_empty_and_a_full_frame():
    z = np.zeros((4, 6), np.uint8)
    for m, target in ((z, R.TO_NONZERO), (z + 9, R.TO_ZERO)):
        d2, near = _both(m, target)
        assert (d2 == R.NONE).all() and (near == -1).all() and R.NONE == api.DT_NONE == 2 ** 31 - 1
        assert np.isposinf(R.root_f32(d2)).all()
    for m, target in ((z + 1, R.TO_NONZERO), (z, R.TO_ZERO)):
        d2, near = _both(m, target)
        assert (d2 == 0).all() and np.array_equal(near.reshape(-1), np.arange(24))


def test_targets_are_complements_and_every_non_zero_byte_is_a_feature():
    rng = np.random.default_rng(5)
    m = rng.choice(np.array([0, 0, 0, 1, 128, 255], np.uint8), size=(9, 12))
    a = _both(m)
    b = _both(np.where(m != 0, 0, 77).astype(np.uint8), R.TO_ZERO)
    c = _both(np.where(m != 0, 255, 0).astype(np.uint8))
    for o in (b, c):
        assert np.array_equal(a[0], o[0]) and np.array_equal(a[1], o[1])


def test_the_restatements_agree_on_random_frames_and_with_scipy():
    from scipy import ndimage
    rng = np.random.default_rng(20261020)
    frames = 0
    for density in (0.0, 0.02, 0.1, 0.5, 1.0):
        for k in range(70):
            h, w = (int(v) for v in rng.integers(1, 14, 2))
            m = np.where(rng.random((h, w)) < density, 255, 0).astype(np.uint8)
            d2, near = _both(m, int(k % 2 and R.TO_ZERO))
            frames += 1
            feat = R.features(m, int(k % 2 and R.TO_ZERO))
            if not feat.any():
                assert (d2 == R.NONE).all() and (near == -1).all()
                continue
            edt = ndimage.distance_transform_edt(~feat)
            assert np.array_equal(d2, np.rint(edt * edt).astype(np.int64))
            # the nearest pixel is a feature pixel at that distance
            yy, xx = np.mgrid[0:h, 0:w]
            ny, nx = near // w, near % w
            assert feat[ny, nx].all() and np.array_equal((xx - nx) ** 2 + (yy - ny) ** 2, d2)
    assert frames == 350


def test_the_float32_rule():
    """HC_DT_F32 is sqrtf((float)d2): above 2^24 the conversion rounds first, and the result is not always the float nearest to the
    root taken in double."""
    v = 77632802   # (float)v is 77632800; the double root of v rounds to the next float up
    got = R.root_f32(np.array([v], np.int32))[0]
    assert np.float32(np.int32(v)) == np.float32(77632800.0)
    assert got == np.sqrt(np.float32(77632800.0)) and got != np.float32(math.sqrt(v))
    assert got.view(np.uint32) == 1175038922
    # exact below 2^24: the nearest float to the real root, as the double route gives it
    rng = np.random.default_rng(3)
    small = np.concatenate([np.arange(0, 4097), rng.integers(0, 1 << 24, 20000), [(1 << 24) - 1, 1 << 24]]).astype(np.int32)
    assert np.array_equal(R.root_f32(small), np.sqrt(small.astype(np.float64)).astype(np.float32))
    # around and above 2^24: by the rule, value by value (python floats are doubles: the conversion through struct is the rounding)
    big = np.concatenate([np.arange((1 << 24) - 40, (1 << 24) + 40), rng.integers(1 << 24, (1 << 31) - 1, 20000), [4099 ** 2 + 1, (1 << 31) - 2]]).astype(np.int32)
    assert np.array_equal(R.root_f32(big), np.sqrt(big.astype(np.float32)))
    differs = R.root_f32(big) != np.sqrt(big.astype(np.float64)).astype(np.float32)
    assert differs.any() and not differs.all()
    assert R.root_f32(np.array([4099 ** 2 + 1], np.int32))[0] == np.float32(4099.0)   # the far corner of a 4100 x 2 frame
    assert np.isposinf(R.root_f32(np.array([R.NONE], np.int32))[0])


# ---- the C ABI -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    build.build()
    return api.load_library()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hipcanny.h")).read(), flags=re.S)


def test_the_symbol_is_exported_by_both_libraries(lib):
    assert NAME in api.ABI_SYMBOLS
    for path in (api.LIB_PATH, build.build_legacy()):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert NAME in {l.split()[-1] for l in out.splitlines() if " T " in l}, path


def test_header_arguments_match_ctypes(lib):
    body = re.search(r"\bint " + NAME + r"\s*\((.*?)\);", _header(), re.S).group(1)
    want = [C.c_void_p if "*" in a else {"int": C.c_int, "size_t": C.c_size_t}[a.strip().rsplit(" ", 1)[0].strip()] for a in body.split(",")]
    assert getattr(lib, NAME).argtypes == want and len(want) == 13
    names = [a.replace("*", " ").split()[-1] for a in body.split(",")]
    assert names == ["ctx", "d_map", "pitch", "frame_stride", "nframes", "target", "dist_type", "d_dist", "dist_pitch", "dist_frame_stride", "d_nearest",
                     "nearest_pitch", "nearest_frame_stride"]


def test_constants_of_the_header_are_the_api_s():
    hdr = _header()
    for body in re.findall(r"enum\s*\{\s*(HC_DT_[^}]*)\}", hdr):
        for item in body.split(","):
            name, value = (t.strip() for t in item.split("="))
            assert getattr(api, name[3:]) == int(value), name
    assert {n for n in re.findall(r"\bHC_(DT_[A-Z0-9_]+)\s*=", hdr)} == {"DT_TO_NONZERO", "DT_TO_ZERO", "DT_SQUARED_I32", "DT_F32"}
    assert int(re.search(r"#define\s+HC_DT_NONE\s+(\d+)", hdr).group(1)) == api.DT_NONE == np.iinfo(np.int32).max


def test_a_null_context_is_refused_under_the_entry_s_name(lib):
    assert getattr(lib, NAME)(*ARGS) == -1
    assert NAME + ": null argument" in api.last_error()


def test_the_test_library_refuses_the_entry():
    build.build_legacy()
    legacy = api.load_library(legacy=True)
    assert getattr(legacy, NAME)(*ARGS) == -1
    assert NAME + ": not part of the test library" in legacy.hc_last_error().decode()
