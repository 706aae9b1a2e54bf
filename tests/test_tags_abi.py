"""tools/tags_abi_check.cpp compiled against the built library and run (no
device): the argument checks of the print_tags calls, and the structure
layouts it prints against the ctypes mirrors of adam_amd/print_tags.py."""
import ctypes
import os
import shutil
import subprocess

from adam_amd import _capi
from adam_amd import print_tags as PT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MIRRORS = {
    "bqsr_tag_counts": (PT._TagCounts, ("counts", "total")),
    "bqsr_tags_chunk": (PT.TagsChunk, ("n_reads", "attr_offsets", "attr_bytes", "attr_validity", "failed",
                                       "failed_validity")),
    "bqsr_tag_value_sizes": (PT._ValueSizes, ("n_runs", "text_bytes")),
    "bqsr_tag_value_host": (PT._ValueHost, ("type", "count", "first_read", "text_offsets", "text")),
}


def test_tags_abi_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "tags_abi_check")
    libdir = os.path.dirname(_capi.LIB_PATH)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "tags_abi_check.cpp"), "-L", libdir, "-ladam_bqsr",
                    "-Wl,-rpath," + libdir, "-o", exe], check=True)
    r = subprocess.run([exe], check=True, capture_output=True, text=True)
    lines = r.stdout.splitlines()
    assert lines[-1] == "tags_abi_check: OK"
    seen = {}
    for l in lines:
        if l.startswith("layout "):
            f = l.split()
            seen[f[1]] = [int(x) for x in f[2:]]
    assert set(seen) == set(MIRRORS)
    for name, (cls, fields) in MIRRORS.items():
        assert seen[name] == [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fields], name


def test_new_symbols_are_listed():
    want = {"bqsr_sam_tag_counts", "bqsr_arrow_tag_counts", "bqsr_sam_tag_values", "bqsr_arrow_tag_values",
            "bqsr_tag_values_fetch", "bqsr_tags_kernel_times"}
    assert want <= set(_capi.EXPORTS)
    lib = ctypes.CDLL(_capi.LIB_PATH)
    assert all(hasattr(lib, n) for n in want)
    assert _capi.STATUS_NAMES[_capi.ATTRIBUTE] == "ATTRIBUTE" and _capi.ATTRIBUTE == 16
