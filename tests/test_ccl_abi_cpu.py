"""The C ABI of hc_connected_components_device without a GPU: the symbol is exported by both libraries; the header's argument
list matches the argtypes api.py gives ctypes; the HC_CC_STAT_* values of the header are api's; a null context is refused under
the entry's name and the test library refuses the entry with its own message."""
import ctypes as C
import os
import re
import subprocess

import pytest

from cudacam_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "hc_connected_components_device"
ARGS = (None, 16, 64, 64 * 48, 1, 8, 4096, 256, 256 * 48, 16, 32, 64, 4)


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


def test_stat_words_of_the_header_are_the_api_s():
    body = re.search(r"enum\s*\{\s*(HC_CC_STAT_LEFT.*?)\}", _header(), re.S).group(1)
    names = [n.split("=")[0].strip() for n in body.split(",")]
    assert names == ["HC_CC_STAT_LEFT", "HC_CC_STAT_TOP", "HC_CC_STAT_WIDTH", "HC_CC_STAT_HEIGHT", "HC_CC_STAT_AREA", "HC_CC_STAT_WORDS"]
    assert body.split(",")[0].replace(" ", "") == "HC_CC_STAT_LEFT=0"   # the rest count up from it
    assert [getattr(api, n[3:]) for n in names] == list(range(6))


def test_a_null_context_is_refused_under_the_entry_s_name(lib):
    assert getattr(lib, NAME)(*ARGS) == -1
    assert NAME + ": null argument" in api.last_error()


def test_the_test_library_refuses_the_entry():
    build.build_legacy()
    legacy = api.load_library(legacy=True)
    assert getattr(legacy, NAME)(*ARGS) == -1
    assert NAME + ": not part of the test library" in legacy.hc_last_error().decode()
