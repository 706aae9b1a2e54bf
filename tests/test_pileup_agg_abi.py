"""tools/pileup_agg_abi_check.cpp compiled against the built library and run
(no device): the argument checks of the pileup aggregation calls, and the
structure layouts it prints against the ctypes mirrors of
adam_amd/aggregate_pileups.py."""
import ctypes
import os
import shutil
import subprocess

from adam_amd import _capi
from adam_amd import aggregate_pileups as AP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MIRRORS = {
    "bqsr_pileup_agg_rows": AP.AggRows,
    "bqsr_pileup_agg_sizes": AP.AggSizes,
    "bqsr_pileup_agg_host": AP.AggHost,
}
SYMBOLS = {"bqsr_pileup_agg_create", "bqsr_pileup_agg_destroy", "bqsr_pileup_agg_add_host", "bqsr_sam_pileup_agg_add",
           "bqsr_arrow_pileup_agg_add", "bqsr_pileup_agg_run", "bqsr_pileup_agg_fetch", "bqsr_pileup_agg_kernel_times"}


def test_pileup_agg_abi_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "pileup_agg_abi_check")
    libdir = os.path.dirname(_capi.LIB_PATH)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "pileup_agg_abi_check.cpp"), "-L", libdir, "-ladam_bqsr",
                    "-Wl,-rpath," + libdir, "-o", exe], check=True)
    r = subprocess.run([exe], check=True, capture_output=True, text=True)
    lines = r.stdout.splitlines()
    assert lines[-1] == "pileup_agg_abi_check: OK"
    seen = {}
    for l in lines:
        if l.startswith("layout "):
            f = l.split()
            seen[f[1]] = [int(x) for x in f[2:]]
    assert set(seen) == set(MIRRORS)
    for name, cls in MIRRORS.items():
        assert seen[name] == [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_], name


def test_field_order_matches_the_header():
    """the mirrors are generated from tables: their field names, in order, are the header's"""
    with open(os.path.join(ROOT, "include", "adam_sam.h")) as fh:
        text = fh.read()
    for name, cls in MIRRORS.items():
        body = text[text.index("typedef struct %s {" % name):text.index("} %s;" % name)]
        fields = [l.split(";")[0].split()[-1].lstrip("*") for l in body.splitlines()[1:] if ";" in l]
        assert fields == [f for f, _ in cls._fields_], name


def test_new_symbols_are_listed():
    assert SYMBOLS <= set(_capi.EXPORTS)
    lib = ctypes.CDLL(_capi.LIB_PATH)
    assert all(hasattr(lib, n) for n in SYMBOLS)
    assert len(_capi.STATUS_NAMES) == 17  # no status code was added
