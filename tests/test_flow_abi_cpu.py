"""The C ABI of hc_pyr_down_device and hc_lk_flow_device without a GPU: the symbols are exported by both libraries; the header's
argument lists match the argtypes api.py gives ctypes; a null context is refused under the entry's name and the test library refuses
both entries with its own message."""
import ctypes as C
import os
import re
import subprocess

import pytest

from cudacam_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {
    "hc_pyr_down_device": (None, 4096, 64, 64 * 48, 64, 48, 65536, 32, 32 * 24, 1),
    "hc_lk_flow_device": (None, 4096, 8192, 64, 64 * 48, 64, 48, 0, 1, 16, 1024, 2048, 8, 21, 30, 0.01, 1e-4, 0, 32, 64),
}


@pytest.fixture(scope="module")
def lib():
    build.build()
    return api.load_library()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hipcanny.h")).read(), flags=re.S)


def test_the_symbols_are_exported_by_both_libraries(lib):
    for path in (api.LIB_PATH, build.build_legacy()):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        have = {l.split()[-1] for l in out.splitlines() if " T " in l}
        for name in ENTRIES:
            assert name in api.ABI_SYMBOLS and name in have, (name, path)


@pytest.mark.parametrize("name, count", [("hc_pyr_down_device", 10), ("hc_lk_flow_device", 20)])
def test_header_arguments_match_ctypes(lib, name, count):
    body = re.search(r"\bint " + name + r"\s*\((.*?)\);", _header(), re.S).group(1)
    kinds = {"int": C.c_int, "size_t": C.c_size_t, "double": C.c_double}
    want = [C.c_void_p if "*" in a else kinds[a.strip().rsplit(" ", 1)[0].strip()] for a in body.split(",")]
    assert getattr(lib, name).argtypes == want and len(want) == count


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_a_null_context_is_refused_under_the_entry_s_name(lib, name):
    assert getattr(lib, name)(*ENTRIES[name]) == -1
    assert name + ": null argument" in api.last_error()


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_the_test_library_refuses_the_entries(name):
    build.build_legacy()
    legacy = api.load_library(legacy=True)
    assert getattr(legacy, name)(*ENTRIES[name]) == -1
    assert name + ": not part of the test library" in legacy.hc_last_error().decode()
