"""`adam flagstat` on the device (bqsr_sam_flagstat, bqsr_flagstat_arrow,
adam_amd/csrc/flagstat.hip, adam_amd/flagstat.py) against the restatement of
the reference (tests/_flagstat_ref.py: core/rdd/FlagStat.scala:21-116,
cli/FlagStat.scala:43-109).  All 36 counts are compared, always."""
import ctypes
import functools
import os
import random
import re

import numpy as np
import pytest

from _adam_ref import convert_sam
from _flagstat_ref import NAMES, flagstat_ref, format_ref, throws
from adam_amd import _capi
from adam_amd import flagstat as FS
from adam_amd import records as R
from adam_amd.bam_writer import sam_to_bam
from adam_amd.sam import SamText
from adam_amd.transform import sam_partitions, transform

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "reference_resources")
FIXTURES = ["artificial.realigned.sam", "artificial.sam", "reads12.sam", "small.sam",
            "small_realignment_targets.sam", "unmapped.sam"]
# the wave (64) and workgroup (256) tails, and more than one workgroup; the grid-stride
# loops: test_flagstat_grid_stride
SIZES = [1, 63, 64, 65, 255, 256, 257, 70001]

SQ = ["chr1", "chr2", "chr3"]
HEADER = b"@HD\tVN:1.4\n" + b"".join(b"@SQ\tSN:%s\tLN:100000000\n" % n.encode() for n in SQ)
NAMES_POOL = ["*", "="] + SQ + ["chrUn"]  # "chrUn" is no @SQ name
MAPQS = [0, 4, 5, 60, 255]


def named(counts):
    return dict(zip(NAMES, counts))


def assert_counts(got, want):
    """got: (failed, passed) FlagStatMetrics; want: the restatement's (failed, passed)"""
    assert named(got[0].counts()) == named(want[0]), "failed"
    assert named(got[1].counts()) == named(want[1]), "passed"


def line(i, flag, rname, mapq, rnext):
    return b"q%d\t%d\t%s\t%d\t%d\t4M\t%s\t%d\t0\tACGT\tIIII\n" % (i, flag, rname.encode(), 1 + i % 977, mapq,
                                                                   rnext.encode(), 1 + i % 911)


def random_records(n, seed):
    """(lines, dicts) of n records: FLAG uniform over all twelve bits (and 0,
    one time in eight), RNAME / RNEXT from NAMES_POOL, MAPQ from MAPQS; the
    reads the reference would throw at are removed by the restatement (the
    rest stays uniform)"""
    rnd = random.Random(seed)
    lines, recs = [], []
    while len(lines) < n:
        cand = []
        for _ in range(n - len(lines) + 8):
            flag = 0 if rnd.randrange(8) == 0 else rnd.randrange(4096)
            cand.append(line(len(lines) + len(cand), flag, rnd.choice(NAMES_POOL), rnd.choice(MAPQS),
                             rnd.choice(NAMES_POOL)))
        for l, r in zip(cand, convert_sam(HEADER + b"".join(cand))):
            if not throws(r):
                lines.append(l)
                recs.append(r)
    return lines[:n], recs[:n]


def random_lines(n, seed):
    return random_records(n, seed)[0]


@functools.lru_cache(maxsize=None)
def generated(n):
    """(SAM text, the records' dicts, the restatement's (failed, passed)); computed once per n"""
    lines, recs = random_records(n, 1000 + n)
    return HEADER + b"".join(lines), recs, flagstat_ref(recs)


def sam_counts(data, bam=False):
    s = SamText(data, bam=bam)
    try:
        return s.flagstat()
    finally:
        s.close()


# ---- fixtures ----------------------------------------------------------------

@pytest.mark.parametrize("name", FIXTURES)
def test_flagstat_reference_fixtures(name):
    data = open(os.path.join(GOLD, name), "rb").read()
    want = flagstat_ref(convert_sam(data))
    assert want[1][0] + want[0][0] > 0
    assert_counts(sam_counts(data), want)
    assert_counts(sam_counts(sam_to_bam(data), bam=True), want)


# ---- generated SAM text ------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_flagstat_generated_sam(n, tmp_path):
    text, recs, want = generated(n)
    if n == SIZES[-1]:  # the input exercises every counter on both sides
        assert all(c > 0 for c in want[0] + want[1])
    assert_counts(sam_counts(text), want)
    # the same through the file entry point, in one partition and in several
    p = tmp_path / "in.sam"
    p.write_bytes(text)
    assert_counts(FS.flagstat(str(p)), want)
    part = max(1, (len(text) - len(HEADER)) // 6)
    n_parts = len(sam_partitions(text, part)[1])
    assert n_parts >= (5 if n >= 63 else 1)  # (one record cannot be cut)
    assert_counts(FS.flagstat(str(p), partition_bytes=part), want)


# ---- NULL_FIELD --------------------------------------------------------------

def test_flagstat_null_field(tmp_path):
    lines = random_lines(400, 7)
    # diffChr with a null mapq: MAPQ 255, and an RNAME outside @SQ against a resolved RNEXT
    lines[137] = line(137, 0x1 | 0x40, "chr1", 255, "chr2")
    lines[301] = line(301, 0x1 | 0x80, "chrUn", 60, "chr3")
    text = HEADER + b"".join(lines)
    recs = convert_sam(text)
    assert [i for i, r in enumerate(recs) if throws(r)] == [137, 301]
    s = SamText(text)
    try:
        with pytest.raises(_capi.BQSRError) as e:
            s.flagstat()
        assert e.value.status == _capi.NULL_FIELD and e.value.read == 137
        # no counts come back
        out = FS._FlagStat()
        ctypes.memset(ctypes.byref(out), 0x55, ctypes.sizeof(out))
        assert FS._lib().bqsr_sam_flagstat(s.ctx.handle, s.h, None, ctypes.byref(out)) == _capi.NULL_FIELD
        assert list(out.passed.c) + list(out.failed.c) == [0] * 36
    finally:
        s.close()
    p = tmp_path / "in.sam"
    p.write_bytes(text)
    for part in (1 << 40, (len(text) - len(HEADER)) // 7):
        assert (part > len(text)) or len(sam_partitions(text, part)[1]) >= 5
        with pytest.raises(_capi.BQSRError) as e:
            FS.flagstat(str(p), partition_bytes=part)
        assert e.value.status == _capi.NULL_FIELD and e.value.read == 137
        assert re.findall(r"read (\d+)", str(e.value)) == ["137"]  # the message names the global ordinal alone
    # with the first one gone, the second is named
    lines[137] = line(137, 0x1 | 0x40, "chr1", 60, "chr2")
    p.write_bytes(HEADER + b"".join(lines))
    with pytest.raises(_capi.BQSRError) as e:
        FS.flagstat(str(p), partition_bytes=(len(text) - len(HEADER)) // 7)
    assert e.value.read == 301


# ---- after MarkDuplicates ----------------------------------------------------

def stacked_text() -> bytes:
    """fragments stacked on a few positions, primary and secondary, with
    unmapped reads between them: MarkDuplicates keeps one per position and
    strand and marks the others"""
    rnd = random.Random(11)
    out = []
    for i in range(160):
        flag = rnd.choice((16, 16, 0x10 | 0x100, 4, 0x200 | 16))
        out.append(b"s%d\t%d\t%s\t%d\t60\t20M\t*\t0\t0\t%s\t%s\n" % (
            i, flag, SQ[rnd.randrange(3)].encode(), 100 * (1 + rnd.randrange(3)), b"ACGT" * 5, b"I" * 20))
    return HEADER + b"".join(out)


def test_flagstat_follows_mark_duplicates():
    text = stacked_text()
    recs = convert_sam(text)
    s = SamText(text)
    try:
        before = s.flagstat()
        assert_counts(before, flagstat_ref(recs))
        assert before[1].dup_primary_total == 0 and before[1].dup_secondary_total == 0
        n_dup = s.mark_duplicates()
        assert n_dup > 0
        dup = (s.batch().flags & R.F_DUPLICATE) != 0
        assert int(dup.sum()) == n_dup
        for r, d in zip(recs, dup):
            r["duplicateRead"] = bool(d)
        want = flagstat_ref(recs)
        after = s.flagstat()
        assert_counts(after, want)
        dups = slice(1, 9)
        assert (after[0].counts()[dups], after[1].counts()[dups]) != (before[0].counts()[dups],
                                                                      before[1].counts()[dups])
        total = sum(after[k].dup_primary_total + after[k].dup_secondary_total for k in (0, 1))
        assert total == n_dup
        # the same once the bits are in the text's FLAG fields
        s.rewrite(None)
        assert_counts(s.flagstat(), want)
        assert_counts(sam_counts(s.text()), want)
    finally:
        s.close()


# ---- the Arrow form through ctypes ---------------------------------------------

BOOLS = FS.BOOL_COLUMNS
INTS = FS.INT_COLUMNS


def bitmap(bits) -> np.ndarray:
    """an Arrow bitmap of ceil(n / 8) bytes; the bits beyond n in the last byte are ones"""
    bits = np.asarray(bits, bool)
    pad = (-len(bits)) % 8
    return np.packbits(np.concatenate([bits, np.ones(pad, bool)]), bitorder="little")


def arrow_chunks(recs, cuts=(1, 63, 130), null_column=None, null_some=None, no_mapq=False):
    """the records as bqsr_flagstat_chunk structures: chunks of `cuts` reads,
    then the rest.  null_column: that boolean column is passed as NULL;
    null_some: (column, mask) -- a validity bitmap nulling the masked reads;
    no_mapq: the mapq column is NULL.  Every buffer is an exact-size numpy
    array (ceil(n / 8) bytes for a bitmap)."""
    keep, chunks = [], []
    a = 0
    bounds = []
    for c in cuts:
        if a + c <= len(recs):
            bounds.append((a, a + c))
            a += c
    if a < len(recs):
        bounds.append((a, len(recs)))

    def ptr(x):
        keep.append(x)
        return x.ctypes.data

    for a, b in bounds:
        C = FS.FlagStatChunk()
        C.n_reads = b - a
        part = recs[a:b]
        for k, name in enumerate(BOOLS):
            if name == null_column:
                continue
            C.bools[k] = ptr(bitmap([r[name] for r in part]))
            if null_some and null_some[0] == name:
                C.bools_validity[k] = ptr(bitmap(~null_some[1][a:b]))
        for name, attr in zip(INTS, ("reference_id", "mate_reference_id", "mapq")):
            if name == "mapq" and no_mapq:
                continue
            vals = [r[name] for r in part]
            # a null slot holds a value that would count if it were read
            setattr(C, attr, ptr(np.array([7 if v is None else v for v in vals], np.int32)))
            if any(v is None for v in vals) or a == 0:
                setattr(C, attr + "_validity", ptr(bitmap([v is not None for v in vals])))
        chunks.append(C)
    return chunks, keep


@pytest.mark.parametrize("n", SIZES)
def test_flagstat_arrow(n):
    _, recs, want = generated(n)
    chunks, keep = arrow_chunks(recs)
    assert sum(c.n_reads for c in chunks) == n
    assert_counts(FS.arrow_flagstat(chunks), want)
    # one boolean column NULL: all false (here in one chunk)
    chunks, keep = arrow_chunks(recs, cuts=(), null_column="properPair")
    assert len(chunks) == 1
    assert_counts(FS.arrow_flagstat(chunks), flagstat_ref([dict(r, properPair=False) for r in recs]))
    # a validity bitmap that nulls some true values: a null boolean reads as false
    mask = np.random.default_rng(n).random(n) < 0.4
    chunks, keep = arrow_chunks(recs, null_some=("readMapped", mask))
    edited = [dict(r, readMapped=r["readMapped"] and not m) for r, m in zip(recs, mask)]
    assert n < 63 or any(r["readMapped"] and m for r, m in zip(recs, mask))
    assert_counts(FS.arrow_flagstat(chunks), flagstat_ref(edited))
    # mapq NULL (all null) on an input with no diffChr read
    quiet = [dict(r, mapq=None) for r in recs if not (r["readPaired"] and r["readMapped"] and r["mateMapped"] and
                                                      r["referenceId"] != r["mateReferenceId"])]
    chunks, keep = arrow_chunks(quiet, no_mapq=True)
    if quiet:
        assert_counts(FS.arrow_flagstat(chunks), flagstat_ref(quiet))
    del keep


def test_flagstat_arrow_empty():
    zero = ((0,) * 18, (0,) * 18)
    assert_counts(FS.arrow_flagstat([]), zero)
    C = FS.FlagStatChunk()
    assert_counts(FS.arrow_flagstat([C, C]), zero)
    assert_counts(sam_counts(HEADER), zero)


def test_flagstat_arrow_null_field():
    _, recs, _ = generated(257)
    recs = [dict(r) for r in recs]
    bad = dict(readPaired=True, readMapped=True, mateMapped=True, referenceId=0, mateReferenceId=1, mapq=None)
    recs[70].update(bad)   # in the third chunk (reads 64 ..)
    recs[200].update(bad)  # in the rest
    chunks, keep = arrow_chunks(recs)
    with pytest.raises(_capi.BQSRError) as e:
        FS.arrow_flagstat(chunks)
    assert e.value.status == _capi.NULL_FIELD and e.value.read == 70  # global over the chunks
    # mapq NULL altogether: the first diffChr read is named
    first = next(i for i, r in enumerate(recs) if r["readPaired"] and r["readMapped"] and r["mateMapped"] and
                 r["referenceId"] != r["mateReferenceId"])
    chunks, keep = arrow_chunks(recs, no_mapq=True)
    with pytest.raises(_capi.BQSRError) as e:
        FS.arrow_flagstat(chunks)
    assert e.value.read == first


def test_flagstat_arrow_device_entry():
    """bqsr_flagstat_arrow_device (the measurement entry of tools/bench_adam.py
    --flagstat): the kernel over buffers already on the device, bitmaps as
    whole 64-bit words, the sums added into the caller's 37 words"""
    import torch
    from adam_amd import bqsr
    n = 257
    _, recs, want = generated(n)
    keep = []

    def words(bits):
        b = bitmap(bits)
        keep.append(torch.from_numpy(np.pad(b, (0, (-len(b)) % 8)).view(np.int64)).cuda())
        return keep[-1].data_ptr()
    C = FS.FlagStatChunk()
    C.n_reads = n
    for k, name in enumerate(BOOLS):
        C.bools[k] = words([r[name] for r in recs])
    for name, attr in zip(INTS, ("reference_id", "mate_reference_id", "mapq")):
        vals = [r[name] for r in recs]
        keep.append(torch.from_numpy(np.array([7 if v is None else v for v in vals], np.int32)).cuda())
        setattr(C, attr, keep[-1].data_ptr())
        setattr(C, attr + "_validity", words([v is not None for v in vals]))
    counters = torch.zeros(37, dtype=torch.int64, device="cuda")
    counters[36] = -1
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ctx = bqsr.Context.get(0)
    for _ in range(2):  # the sums are added into the block
        _capi.check(FS._lib().bqsr_flagstat_arrow_device(ctx.handle, ctypes.byref(C), counters.data_ptr(), sp))
    torch.cuda.synchronize()
    got = counters.cpu().tolist()
    assert named(got[:18]) == named(tuple(2 * c for c in want[1]))
    assert named(got[18:36]) == named(tuple(2 * c for c in want[0]))
    assert got[36] == -1


# ---- the grid-stride loops -------------------------------------------------------
# BQSR_TUNE_FLAGSTAT_GRID caps the kernels' grids, so that the 70 001 reads
# (1094 groups of 64, 18 tiles of 64 groups) take every wavefront through many
# passes.  One workgroup (4 waves): flagstat_sam makes 273 or 274 passes per
# wave -- its lanes fill and are counted four times, then 17 or 18 lanes are
# left for the tail -- and flagstat_arrow 4 or 5.  Three workgroups (12
# waves): 91 or 92 passes, one full set of lanes and a tail of 27 or 28.

N_STRIDE = SIZES[-1]


@pytest.mark.parametrize("grid", [1, 3])
def test_flagstat_grid_stride(grid):
    from adam_amd import bqsr
    text, recs, want = generated(N_STRIDE)
    with bqsr.Context.get(0).tuned(flagstat_grid=grid):
        assert_counts(sam_counts(text), want)
        chunks, keep = arrow_chunks(recs)
        assert_counts(FS.arrow_flagstat(chunks), want)
        chunks, keep = arrow_chunks(recs, cuts=())
        assert_counts(FS.arrow_flagstat(chunks), want)


def test_flagstat_null_field_later_pass():
    """a throwing read met in a later pass: with one workgroup, read 40 123
    (group 626) is wave 2's pass 156 -- lane 28 after two full sets of lanes --
    and read 69 990 (group 1093) is in wave 1's tail; for flagstat_arrow they
    are in tiles 9 and 17"""
    from adam_amd import bqsr
    text, recs, _ = generated(N_STRIDE)
    lines = text[len(HEADER):].splitlines(keepends=True)
    recs = [dict(r) for r in recs]
    first, second = 40_123, 69_990
    bad = dict(readPaired=True, readMapped=True, mateMapped=True, referenceId=0, mateReferenceId=1, mapq=None)
    with bqsr.Context.get(0).tuned(flagstat_grid=1):
        for want in (first, second):
            for i in (first, second):
                if i >= want:
                    lines[i] = line(i, 0x1 | 0x40, "chr1", 255, "chr2")
                    recs[i].update(bad)
            assert throws(convert_sam(HEADER + lines[want])[0])
            with pytest.raises(_capi.BQSRError) as e:
                sam_counts(HEADER + b"".join(lines))
            assert e.value.status == _capi.NULL_FIELD and e.value.read == want
            chunks, keep = arrow_chunks(recs)
            with pytest.raises(_capi.BQSRError) as e:
                FS.arrow_flagstat(chunks)
            assert e.value.status == _capi.NULL_FIELD and e.value.read == want
            # the next round: this one no longer throws
            lines[want] = line(want, 0x1 | 0x40, "chr1", 60, "chr2")
            recs[want].update(mapq=60)


# ---- Parquet and the command ----------------------------------------------------

def test_flagstat_parquet(tmp_path):
    import pyarrow.parquet as pq
    text, recs, want = generated(257)
    src, out = tmp_path / "in.sam", tmp_path / "out.adam"
    src.write_bytes(text)
    transform(str(src), str(out))
    assert_counts(FS.flagstat(str(out)), want)
    assert_counts(FS.flagstat(str(src)), want)
    # duplicateRead missing from the file: passed as NULL, all false
    table = pq.ParquetDataset(str(out)).read()
    assert "duplicateRead" in table.column_names
    lean = tmp_path / "lean.parquet"
    pq.write_table(table.drop(["duplicateRead"]), str(lean), row_group_size=100)
    edited = [dict(r, duplicateRead=False) for r in recs]
    assert flagstat_ref(edited) != want
    assert_counts(FS.flagstat(str(lean)), flagstat_ref(edited))


@pytest.mark.parametrize("kind", ["sam", "bam", "adam"])
def test_flagstat_cli(kind, tmp_path, capsys):
    data = open(os.path.join(GOLD, "small_realignment_targets.sam"), "rb").read()
    want = format_ref(*flagstat_ref(convert_sam(data))) + "\n"
    src = tmp_path / "in.sam"
    src.write_bytes(data)
    path = src
    if kind == "bam":
        path = tmp_path / "in.bam"
        path.write_bytes(sam_to_bam(data))
    elif kind == "adam":
        path = tmp_path / "in.adam"
        transform(str(src), str(path))
    capsys.readouterr()
    assert FS.main([str(path)]) == 0
    cap = capsys.readouterr()
    assert cap.out == want
    assert cap.err.startswith("reads=%d " % len(convert_sam(data))) and "phases=" in cap.err


def test_flagstat_cli_generated(tmp_path, capsys):
    text, _, want = generated(257)
    p = tmp_path / "in.sam"
    p.write_bytes(text)
    assert FS.main([str(p), "-partition_bytes", "4000"]) == 0
    assert capsys.readouterr().out == format_ref(*want) + "\n"
