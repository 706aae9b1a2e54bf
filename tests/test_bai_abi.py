"""The BAM index calls of the C ABI without a device: the symbols are exported
and listed, the ctypes mirror matches the header's structure (names from the
header's text, sizes and offsets from a compiler), the argument checks answer
before any device call, and -bam_index without a .bam output is refused before
the input is opened."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from adam_amd import _capi
from adam_amd import transform as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"bqsr_bam_index_create", "bqsr_bam_index_destroy", "bqsr_bam_index_add", "bqsr_bam_index_set_members",
           "bqsr_bam_index_finish", "bqsr_bam_index_size", "bqsr_bam_index_bytes", "bqsr_bam_index_kernel_times"}


def header_fields(name):
    with open(os.path.join(ROOT, "include", "adam_sam.h")) as fh:
        text = fh.read()
    body = text[text.index("typedef struct %s {" % name):text.index("} %s;" % name)]
    return [l.split(";")[0].split()[-1].lstrip("*") for l in body.splitlines()[1:] if ";" in l]


def test_new_symbols_are_listed():
    # (the measurement-only times call is exported and bound, not listed: tests/test_kernel_times.py pins the
    # listed *_times calls to the eight that read a thread's last job, and this one reads an index's own)
    assert SYMBOLS - {"bqsr_bam_index_kernel_times"} <= set(_capi.EXPORTS) and SYMBOLS == set(T._INDEX_SIG)
    lib = ctypes.CDLL(_capi.LIB_PATH)
    assert all(hasattr(lib, n) for n in SYMBOLS)
    assert len(_capi.STATUS_NAMES) == 17 and _capi.UNSORTED == 17  # the refusals reuse mpileup's status


def test_sizes_mirror_matches_the_header_and_the_compiler(tmp_path):
    name, cls = "bqsr_bam_index_sizes", T.BamIndexSizes
    fields = header_fields(name)
    assert fields == [f for f, _ in cls._fields_]
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    src = ['#include <cstddef>', '#include <cstdio>', '#include "adam_sam.h"', 'int main() {',
           '  std::printf("%%zu", sizeof(%s));' % name]
    src += ['  std::printf(" %%zu", offsetof(%s, %s));' % (name, f) for f in fields]
    src += ['  return 0;', '}']
    path = str(tmp_path / "layout.cpp")
    with open(path, "w") as fh:
        fh.write("\n".join(src) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), path, "-o", exe],
                   check=True)
    seen = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert seen == [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]


def test_argument_checks_without_a_device():
    L = T._index_lib()
    fake = ctypes.c_void_p(8)  # never dereferenced: another argument is refused first
    bad = _capi.INVALID_ARG
    h = ctypes.c_void_p()
    sz = T.BamIndexSizes()
    table = np.zeros(4, np.uint64)
    buf = np.zeros(8, np.uint8)
    ms = (ctypes.c_double * len(T.BAM_INDEX_KERNELS))()
    assert L.bqsr_bam_index_create(None, 1, ctypes.byref(h)) == bad
    assert L.bqsr_bam_index_create(fake, -1, ctypes.byref(h)) == bad
    assert L.bqsr_bam_index_create(fake, 1, None) == bad
    assert b"bqsr_bam_index_create: bad arguments" in L.bqsr_last_error()
    assert L.bqsr_bam_index_add(None, fake, 0, None) == bad
    assert L.bqsr_bam_index_add(fake, None, 0, None) == bad
    assert L.bqsr_bam_index_add(fake, fake, -1, None) == bad
    assert L.bqsr_bam_index_set_members(None, table.ctypes.data, 1, None) == bad
    assert L.bqsr_bam_index_set_members(fake, None, 1, None) == bad
    assert L.bqsr_bam_index_set_members(fake, table.ctypes.data, 0, None) == bad
    assert L.bqsr_bam_index_finish(None, None) == bad
    assert L.bqsr_bam_index_size(None, ctypes.byref(sz)) == bad and L.bqsr_bam_index_size(fake, None) == bad
    assert L.bqsr_bam_index_bytes(None, buf.ctypes.data, 8) == bad
    assert L.bqsr_bam_index_bytes(fake, None, 8) == bad
    assert L.bqsr_bam_index_bytes(fake, buf.ctypes.data, -1) == bad
    assert L.bqsr_bam_index_kernel_times(None, ms) == bad and L.bqsr_bam_index_kernel_times(fake, None) == bad
    L.bqsr_bam_index_destroy(None)
    # create and the member table's checks need no device either
    assert L.bqsr_bam_index_create(fake, 3, ctypes.byref(h)) == 0
    try:
        assert L.bqsr_bam_index_finish(h, None) == bad and b"before bqsr_bam_index_set_members" in L.bqsr_last_error()
        assert L.bqsr_bam_index_size(h, ctypes.byref(sz)) == bad
        for t in ([5, 0, 10, 28],           # the stream does not start at 0
                  [0, 0, 70000, 28],        # a member above 65536 bytes
                  [0, 28, 10, 28]):         # file offsets that do not ascend
            assert L.bqsr_bam_index_set_members(h, np.array(t, np.uint64).ctypes.data, 1, None) == bad, t
        assert L.bqsr_bam_index_kernel_times(h, ms) == 0 and list(ms) == [0.0] * len(T.BAM_INDEX_KERNELS)
    finally:
        L.bqsr_bam_index_destroy(h)  # (no call selected the context's device: the context is not read)


def test_member_walk():
    from adam_amd.sam import BGZF_EOF, bgzf_compress
    data = bgzf_compress(bytes(70000), 6) + bgzf_compress(b"xyz", 0)
    table = []
    s, f = T.bgzf_member_table(data, 0, 0, table)
    s, f = T.bgzf_member_table(BGZF_EOF, s, f, table)
    sizes = [len(bgzf_compress(bytes(65280), 6)), len(bgzf_compress(bytes(4720), 6)), 3 + 31]
    assert table == [0, 0, 65280, sizes[0], 70000, sizes[0] + sizes[1], 70003, sum(sizes)]
    assert (s, f) == (70003, sum(sizes) + 28)
    with pytest.raises(ValueError):
        T.bgzf_member_table(data[:-3], 0, 0, [])


def test_cli_refuses_before_the_input_is_opened(tmp_path, capsys):
    missing = str(tmp_path / "no_such_input.sam")
    with pytest.raises(SystemExit):
        T.main([missing, str(tmp_path / "out.sam"), "-bam_index"])
    assert "-bam_index applies to BAM output only" in capsys.readouterr().err
    with pytest.raises(ValueError, match="-bam_index applies to BAM output only"):
        T.transform(missing, str(tmp_path / "out.adam"), bam_index=True)
    # an existing index is refused as an existing BAM is, before the input is opened
    out = tmp_path / "out.bam"
    (tmp_path / "out.bam.bai").write_bytes(b"old")
    with pytest.raises(FileExistsError):
        T.transform(missing, str(out), bam_index=True)
    assert (tmp_path / "out.bam.bai").read_bytes() == b"old" and not os.path.exists(str(out) + ".partial")
