"""tools/parquet_pages_abi_check.cpp compiled against the built library and
run (no device): the argument checks of the page encoder's calls, and the
structure layouts it prints against the ctypes mirrors of
adam_amd/parquet_pages.py."""
import ctypes
import os
import shutil
import subprocess
import threading

from adam_amd import _capi
from adam_amd import parquet_pages as PP
from adam_amd import reads2ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MIRRORS = {
    "bqsr_parquet_column": PP.ParquetColumn,
    "bqsr_parquet_page": PP.ParquetPage,
    "bqsr_parquet_pages_sizes": PP.PagesSizes,
}
SYMBOLS = {"bqsr_parquet_pages_create", "bqsr_parquet_pages_destroy", "bqsr_parquet_pages_size",
           "bqsr_parquet_pages_emit", "bqsr_parquet_pages_minmax", "bqsr_parquet_pages_kernel_times",
           "bqsr_sam_pileup_device_columns", "bqsr_arrow_pileup_device_columns", "bqsr_sam_pileup_read_spans",
           "bqsr_arrow_pileup_read_spans"}


def test_parquet_pages_abi_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "parquet_pages_abi_check")
    libdir = os.path.dirname(_capi.LIB_PATH)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "parquet_pages_abi_check.cpp"), "-L", libdir, "-ladam_bqsr",
                    "-Wl,-rpath," + libdir, "-o", exe], check=True)
    r = subprocess.run([exe], check=True, capture_output=True, text=True)
    lines = r.stdout.splitlines()
    assert lines[-1] == "parquet_pages_abi_check: OK"
    seen = {}
    for l in lines:
        if l.startswith("layout "):
            f = l.split()
            seen[f[1]] = [int(x) for x in f[2:]]
    assert set(seen) == set(MIRRORS)
    for name, cls in MIRRORS.items():
        assert seen[name] == [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_], name


def test_field_order_matches_the_header():
    with open(os.path.join(ROOT, "include", "adam_sam.h")) as fh:
        text = fh.read()
    for name, cls in MIRRORS.items():
        body = text[text.index("typedef struct %s {" % name):text.index("} %s;" % name)]
        fields = [l.split(";")[0].split()[-1].lstrip("*") for l in body.splitlines()[1:] if ";" in l]
        assert fields == [f for f, _ in cls._fields_], name
    assert (PP.PLAIN_INT32, PP.PLAIN_INT64, PP.DICT_INDEX) == (0, 1, 2)


def test_new_symbols_are_listed_and_bound():
    # (the MEASUREMENT-ONLY times call is exported and bound by its module, and, like bqsr_bam_index_kernel_times,
    # not among _capi.EXPORTS, whose *_times entries tests/test_kernel_times.py enumerates)
    assert SYMBOLS - {"bqsr_parquet_pages_kernel_times"} <= set(_capi.EXPORTS)
    lib = ctypes.CDLL(_capi.LIB_PATH)
    assert all(hasattr(lib, n) for n in SYMBOLS)
    assert SYMBOLS == set(PP._SIG) | {n for n in R._SIG if n.endswith(("device_columns", "read_spans"))}
    assert len(_capi.STATUS_NAMES) == 17  # no status code was added
    assert PP.KERNELS == ("size", "emit")
    seen = []  # a thread that ran no encode reads zeros
    t = threading.Thread(target=lambda: seen.append(PP.kernel_times()))
    t.start()
    t.join()
    assert seen == [(0.0, 0.0)]


def test_the_flag_is_parsed_and_the_default_is_the_host(tmp_path):
    import inspect
    import pytest
    assert inspect.signature(R.reads2ref).parameters["parquet_encoder"].default == "host"
    assert inspect.signature(R._reads2ref).parameters["parquet_encoder"].default == "host"
    with pytest.raises(SystemExit):
        R.main(["in.sam", str(tmp_path / "o.adam"), "-parquet_encoder", "elsewhere"])
    assert os.listdir(str(tmp_path)) == []
