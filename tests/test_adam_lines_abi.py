"""adam2sam's calls of the C ABI without a device: the symbols are exported,
the ctypes mirror of bqsr_adam_lines_chunk matches the header's structure
(names from the header's text, sizes and offsets from a compiler), the
argument checks answer before any device call, and the command's own refusals
come before the input is opened."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from adam_amd import _capi, adam2sam as A, parquet as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"bqsr_arrow_sam_lines", "bqsr_adam_lines_kernel_times"}


def header_fields(name):
    """the declarators of a struct of include/adam_sam.h, in order"""
    with open(os.path.join(ROOT, "include", "adam_sam.h")) as fh:
        text = fh.read()
    body = text[text.index("typedef struct %s {" % name):text.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split("{", 1)[1].split(";"):
        if decl.strip():
            first, *more = decl.split(",")
            out += [re.sub(r"\[.*\]", "", d.split()[-1].lstrip("*")) for d in [first] + more]
    return out


def test_symbols_are_exported_and_bound():
    # (the measurement-only times call is exported and bound, not listed: tests/test_kernel_times.py pins the listed
    # *_times calls to those that take one double* a stage of a fixed list)
    assert "bqsr_arrow_sam_lines" in _capi.EXPORTS and SYMBOLS == set(P._LINES_SIG)
    lib = ctypes.CDLL(_capi.LIB_PATH)
    assert all(hasattr(lib, n) for n in SYMBOLS)


def test_chunk_mirror_matches_the_header_and_the_compiler(tmp_path):
    name, cls = "bqsr_adam_lines_chunk", P._LinesChunk
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
    # the boolean columns are adam_save's, in its order
    from adam_amd.adam_save import BOOL_COLS
    assert len(BOOL_COLS) == 11 and cls.bools.size == cls.bools_validity.size == 11 * ctypes.sizeof(ctypes.c_void_p)


def test_argument_checks_without_a_device():
    L = P._lines_lib()
    fake = ctypes.c_void_p(8)  # never dereferenced: another argument is refused first
    bad = _capi.INVALID_ARG
    h = ctypes.c_void_p()
    one = (P._LinesChunk * 1)()
    off = np.array([0, 3], np.int64)
    blob = np.frombuffer(b"chr", np.uint8)
    call = lambda ctx, ch, n, b, o, nr, hd, out: L.bqsr_arrow_sam_lines(  # noqa: E731
        ctx, ch, n, b, o, nr, hd, len(hd), None, out)
    assert call(None, one, 0, None, None, 0, b"", ctypes.byref(h)) == bad
    assert b"bqsr_arrow_sam_lines: bad arguments" in L.bqsr_last_error()
    assert call(fake, one, 0, None, None, 0, b"", None) == bad
    assert call(fake, one, -1, None, None, 0, b"", ctypes.byref(h)) == bad
    assert call(fake, None, 1, None, None, 0, b"", ctypes.byref(h)) == bad
    assert call(fake, one, 0, blob.ctypes.data, None, 1, b"", ctypes.byref(h)) == bad
    assert call(fake, one, 0, None, off.ctypes.data, 1, b"", ctypes.byref(h)) == bad
    assert b"bad reference name offsets" in L.bqsr_last_error()
    down = np.array([3, 0], np.int64)
    assert call(fake, one, 0, blob.ctypes.data, down.ctypes.data, 1, b"", ctypes.byref(h)) == bad
    one[0].n_reads = -1
    assert call(fake, one, 1, None, None, 0, b"", ctypes.byref(h)) == bad
    assert b"negative chunk length" in L.bqsr_last_error()
    one[0].n_reads = 1
    offs = np.array([4, 2], np.int32)
    one[0].qual = P._Strings(offs.ctypes.data, None, None)
    assert call(fake, one, 1, None, None, 0, b"", ctypes.byref(h)) == bad
    assert b"bad string offsets" in L.bqsr_last_error()
    one[0].qual = P._Strings(None, None, None)
    # the header holds header lines only, and its @RG / @SQ lines are complete
    assert call(fake, one, 1, None, None, 0, b"@SQ\tSN:c\nr\t0\t*\n", ctypes.byref(h)) == bad
    assert b"not a header line" in L.bqsr_last_error()
    assert call(fake, one, 1, None, None, 0, b"@SQ\tLN:5\n", ctypes.byref(h)) == _capi.SAM_PARSE
    assert not h
    ms = [ctypes.c_double(-1.0) for _ in P.LINES_STAGES]
    assert L.bqsr_adam_lines_kernel_times(*[ctypes.byref(v) for v in ms]) == 0
    assert L.bqsr_adam_lines_kernel_times(None, None, None, None) == 0


def test_command_refuses_before_the_input_is_opened(tmp_path, capsys):
    missing = str(tmp_path / "no_such_input.adam")
    for argv, msg in (([missing, str(tmp_path / "o.sam"), "-bam_index"], "-bam_index applies to BAM output only"),
                      ([missing, str(tmp_path / "o.sam"), "-bam_compressor", "device"], "-bam_compressor applies"),
                      ([missing, str(tmp_path / "o.bam"), "-bam_compressor", "device", "-bam_compression_level", "3"],
                       "one level")):
        with pytest.raises(SystemExit):
            A.main(argv)
        assert msg in capsys.readouterr().err
    with pytest.raises(ValueError, match="-bam_index applies to BAM output only"):
        A.adam2sam(missing, str(tmp_path / "o.sam"), bam_index=True)
    with pytest.raises(ValueError, match="reads ADAM Parquet"):
        A.adam2sam(str(tmp_path / "in.sam"), str(tmp_path / "o.sam"))
    (tmp_path / "o.bam").write_bytes(b"old")
    with pytest.raises(FileExistsError):
        A.adam2sam(missing, str(tmp_path / "o.bam"))
    assert sorted(os.listdir(str(tmp_path))) == ["o.bam"] and (tmp_path / "o.bam").read_bytes() == b"old"


def test_header_readers(tmp_path):
    from adam_amd.sam import BGZF_EOF, bgzf_compress
    head = b"@HD\tVN:1.4\n@SQ\tSN:chr1\tLN:100000\n@SQ\tSN:chr2\tLN:5\n" * 1 + b"@CO\t" + b"x" * 70000 + b"\n"
    (tmp_path / "h.sam").write_bytes(head + b"r\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\n@CO\tnot a header line\n")
    assert A.read_header(str(tmp_path / "h.sam")) == head
    import struct
    refs = b"".join(struct.pack("<i", len(n) + 1) + n + b"\0" + struct.pack("<i", ln)
                    for n, ln in ((b"chr1", 100000), (b"chr2", 5)))
    stream = b"BAM\1" + struct.pack("<i", len(head) + 2) + head + b"\0\0" + struct.pack("<i", 2) + refs
    (tmp_path / "h.bam").write_bytes(bgzf_compress(stream, 6) + BGZF_EOF)  # two members hold the text
    assert A.read_header(str(tmp_path / "h.bam")) == head
    assert P.header_sq_names(head) == ["chr1", "chr2"]
    (tmp_path / "bad.bam").write_bytes(bgzf_compress(b"BAX\1" + bytes(8), 6))
    with pytest.raises(ValueError, match="no BAM magic"):
        A.read_header(str(tmp_path / "bad.bam"))


def test_synthesised_header_equals_the_restatement():
    import _adam_lines_ref as R
    from _adam_ref import convert_sam
    recs = convert_sam(R.canonical_sam(300), R.run_date) + [{}]
    assert P.sam_header(R.table(recs, cuts=(7, 130))) == R.header(recs)
    assert P.sam_header(R.table([])) == b"" and P.sam_header(R.table([{}])) == b""
    t = R.table(recs).drop_columns(["referenceUrl", "mateReferenceUrl", "recordGroupRunDateEpoch"])
    assert b"UR:" not in P.sam_header(t) and b"DT:" not in P.sam_header(t) and b"LN:200000000" in P.sam_header(t)
    for a, b, what in ((dict(referenceId=0, referenceName="x"), dict(referenceId=0, referenceName="y"), "two names"),
                       (dict(referenceId=0, referenceName="x"), dict(mateReferenceId=1, mateReference="x"), "two ids"),
                       (dict(referenceId=0, referenceName="x", referenceLength=5),
                        dict(referenceId=0, referenceName="x", referenceLength=6), "two lengths"),
                       (dict(recordGroupName="g", recordGroupSample="a"),
                        dict(recordGroupName="g", recordGroupSample="b"), "two values of recordGroupSample")):
        with pytest.raises(ValueError, match=what) as e:
            P.sam_header(R.table([a, {}, b]))
        assert "'x'" in str(e.value) or "'g'" in str(e.value) or "id 0" in str(e.value)
    # ids need not be dense, and order the lines
    recs = [dict(referenceId=7, referenceName="b", referenceLength=9), dict(mateReferenceId=2, mateReference="z")]
    assert P.sam_header(R.table(recs)) == R.header(recs) == b"@SQ\tSN:z\n@SQ\tSN:b\tLN:9\n"
