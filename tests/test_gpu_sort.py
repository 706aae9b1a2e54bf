"""`transform -sort_reads` on the device (bqsr_sort_order, bqsr_sam_sort,
adam_amd/csrc/sam_sort.hip) against the restatement of the reference's sort
(tests/_sort_ref.py: core/rdd/AdamRDDFunctions.scala:63-93,
models/ReferencePosition.scala:73-95,155-166)."""
import os
import random

import numpy as np
import pytest

from _sort_ref import sam_keys, sort_order_ref, sorted_sam, split_sam, suite_reads
from adam_amd import _capi, synth
from adam_amd import records as R
from adam_amd.bam_writer import sam_to_bam
from adam_amd.records import read_sam
from adam_amd.sam import SamText, sort_order
from adam_amd.samgen import sam_text
from adam_amd.transform import main, transform, transform_parquet

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "reference_resources")
FIXTURES = ["artificial.realigned.sam", "artificial.sam", "reads12.sam", "small.sam",
            "small_realignment_targets.sam", "unmapped.sam"]
SORTED_FIXTURES = ["artificial.realigned.sam", "artificial.sam", "small_realignment_targets.sam"]
COLS = ["flags", "rg_id", "ref_index", "start", "seq_offset", "seq", "qual_offset", "qual", "cigar_offset", "cigar",
        "md_offset", "md"]


def assert_same_columns(a: R.RecordBatch, b: R.RecordBatch):
    assert a.n_reads == b.n_reads
    assert a.ref_names == b.ref_names
    for c in COLS:
        x, y = getattr(a, c), getattr(b, c)
        assert x.dtype == y.dtype and np.array_equal(x, y), c


def expected_text(data: bytes, bam: bool = False) -> bytes:
    """a second parse of the same bytes, its text as rewrite(None) emits it,
    the record lines permuted by the reference's order"""
    s = SamText(data, bam=bam)
    try:
        s.rewrite(None)
        return sorted_sam(s.text())
    finally:
        s.close()


def check_sort(data: bytes, tmp_path, bam: bool = False):
    """sort() gives the expected text byte for byte, and the handle is the
    parse of that text"""
    want = expected_text(data, bam)
    s = SamText(data, bam=bam)
    try:
        s.sort()
        got = s.text()
        assert got == want
        p = tmp_path / "sorted.sam"
        p.write_bytes(got)
        assert_same_columns(s.batch(), read_sam(str(p)))
        assert s.counts().text_bytes == len(want)
    finally:
        s.close()
    return want


def reversed_records(text: bytes) -> bytes:
    header, lines = split_sam(text)
    return header + b"".join(l + b"\n" for l in reversed(lines))


@pytest.mark.parametrize("name", FIXTURES)
def test_sort_reference_fixtures(name, tmp_path):
    check_sort(open(os.path.join(GOLD, name), "rb").read(), tmp_path)


@pytest.mark.parametrize("name", SORTED_FIXTURES)
def test_sort_reference_fixtures_reversed(name, tmp_path):
    text = reversed_records(open(os.path.join(GOLD, name), "rb").read())
    want = check_sort(text, tmp_path)
    assert want != text  # (records move)


@pytest.mark.parametrize("name", ["reads12.sam", "small.sam"])
def test_sort_bam(name, tmp_path):
    check_sort(sam_to_bam(open(os.path.join(GOLD, name), "rb").read()), tmp_path, bam=True)


# ---- synthetic text ----------------------------------------------------------

SQ = ["ref%02d" % i for i in range(100)]
HEADER = b"@HD\tVN:1.4\n" + b"".join(b"@SQ\tSN:%s\tLN:100000000\n" % n.encode() for n in SQ)


def rec(name, flag, ref, pos, n_bases=8, end=b"\n", tags=b""):
    """one record line; ref: an @SQ index, a name, or None ('*'); pos 1-based (0: none)"""
    rname = b"*" if ref is None else (SQ[ref].encode() if isinstance(ref, int) else ref)
    seq = (b"ACGT" * (n_bases // 4 + 1))[:n_bases]
    cigar = b"%dM" % n_bases
    return b"%s\t%d\t%s\t%d\t60\t%s\t*\t0\t0\t%s\t%s%s%s" % (name, flag, rname, pos, cigar, seq, b"I" * n_bases,
                                                           tags, end)


def suite_text(n=1000, seed=20131107) -> bytes:
    mapped, ref, start = suite_reads(seed, n)
    return HEADER + b"".join(rec(b"q%d" % i, 16 if m else 4, ref[i] if m else None, start[i] + 1 if m else 0)
                             for i, m in enumerate(mapped))


def mixed_text(n, seed) -> bytes:
    """n reads: mapped on few positions (ties), FLAG 0 and 0x4 reads with coordinates, plain unmapped ones"""
    rnd = random.Random(seed)
    out = [HEADER]
    for i in range(n):
        kind = rnd.randrange(5)
        ref, pos = rnd.randrange(3), 1 + rnd.randrange(4)
        if kind <= 1:
            out.append(rec(b"m%d" % i, rnd.choice((16, 1, 99, 256, 1024)), ref, pos, 1 + rnd.randrange(40)))
        elif kind == 2:
            out.append(rec(b"z%d" % i, 0, ref, pos, 1 + rnd.randrange(40)))       # Q2: not mapped
        elif kind == 3:
            out.append(rec(b"u%d" % i, 4 | 1 | 8, ref, pos, 1 + rnd.randrange(40)))  # the mate's coordinates
        else:
            out.append(rec(b"x%d" % i, 4, None, 0, 1 + rnd.randrange(40)))
    return b"".join(out)


def residues_text() -> bytes:
    """line lengths (with the newline) of every residue mod 16, each at an
    even and at an odd start offset; the names pad the lines, a line of odd
    length flips the parity when no wanted pair starts here"""
    base = len(rec(b"", 16, 5, 2000))
    need = {(r, p) for r in range(16) for p in range(2)}
    out, at, i = [HEADER], len(HEADER), 0
    while need:
        here = sorted(r for r, p in need if p == at % 2)
        r = here[0] if here else 1
        k = 1 + (r - base - 1) % 16 + 16 * (i % 3)  # at least one name byte
        line = rec(b"n" * k, 16, (7 * i) % 100, 2000 - i)
        assert len(line) % 16 == r
        need.discard((r, at % 2))
        out.append(line)
        at += len(line)
        i += 1
    return b"".join(out)


def lengths_text() -> bytes:
    """1-base and 10 000-base reads in one file (longer than the gather's pieces), 4096-byte boundary cases"""
    out = [HEADER]
    for i, nb in enumerate((1, 10000, 1, 1, 10000, 2000, 1, 10000, 2031, 2032, 2033, 2034, 1, 4075, 4076, 4077)):
        out.append(rec(b"L%d" % i, 16 if i % 3 else 4, 7 - i % 4, 100 - i, nb))
    return b"".join(out)


def wrap_text() -> bytes:
    """10 003 short unmapped records and three mapped ones (the counter wraps at 10 001)"""
    out = [HEADER]
    for i in range(10006):
        if i in (5, 5000, 10005):
            out.append(rec(b"m%d" % i, 16, 1, 10 - i % 3, 4))
        else:
            out.append(rec(b"u%d" % i, 4, None, 0, 4))
    return b"".join(out)


SYNTHETIC = {
    "suite_1000": suite_text,
    "ties_flag0_0x4": lambda: mixed_text(500, 3),
    "lengths_1_and_10000": lengths_text,
    "residues_mod_16": residues_text,
    "no_final_newline": lambda: mixed_text(130, 5)[:-1],
    "crlf": lambda: HEADER + mixed_text(131, 6)[len(HEADER):].replace(b"\n", b"\r\n"),
    "empty_lines": lambda: HEADER + mixed_text(70, 8)[len(HEADER):].replace(b"\n", b"\n\n", 9),
    "header_only": lambda: HEADER,
    "one_read": lambda: HEADER + rec(b"only", 16, 4, 9),
    "one_read_unmapped_no_newline": lambda: HEADER + rec(b"only", 4, None, 0, end=b""),
    "all_mapped": lambda: HEADER + b"".join(rec(b"q%d" % i, 16, (i * 37) % 100, 1 + (i * 101) % 977, 1 + i % 50)
                                            for i in range(300)),
    "all_unmapped": lambda: HEADER + b"".join(rec(b"q%d" % i, 4, None, 0, 1 + i % 50) for i in range(300)),
    "n63": lambda: mixed_text(63, 63),
    "n64": lambda: mixed_text(64, 64),
    "n65": lambda: mixed_text(65, 65),
    "n257": lambda: mixed_text(257, 257),
    "counter_wrap": wrap_text,
}


@pytest.mark.parametrize("case", sorted(SYNTHETIC))
def test_sort_synthetic(case, tmp_path):
    text = SYNTHETIC[case]()
    want = check_sort(text, tmp_path)
    if case == "counter_wrap":
        # descending c, ties in input order; by 1-based ordinal among the unmapped reads:
        # 10000 .. 3 (c = ordinal), 2 and 10003 (c = 2), 1 and 10002 (c = 1), 10001 (c = 0)
        names = [l.split(b"\t")[0] for l in split_sam(want)[1]]
        unm = [l.split(b"\t")[0] for l in split_sam(text)[1] if l.startswith(b"u")]
        assert names[3:] == unm[9999:1:-1] + [unm[1], unm[10002], unm[0], unm[10001], unm[10000]]
    if case == "residues_mod_16":  # every (length mod 16, start offset parity) occurs in the input
        header, lines = split_sam(text)
        seen, at = set(), len(header)
        for l in lines:
            seen.add(((len(l) + 1) % 16, at % 2))
            at += len(l) + 1
        assert len(seen) == 32


# ---- bqsr_sort_order ---------------------------------------------------------

def as_columns(mapped, ref, start):
    flags = np.array([(R.F_MAPPED if m else 0) | (R.F_HAS_START if s is not None else 0)
                      for m, s in zip(mapped, start)], np.uint32)
    return (flags, np.array([-1 if r is None else r for r in ref], np.int32),
            np.array([0 if s is None else s for s in start], np.int64))


def test_sort_order_suite_shape():
    mapped, ref, start = suite_reads()
    assert sort_order(*as_columns(mapped, ref, start)).tolist() == sort_order_ref(mapped, ref, start)


def test_sort_order_counter_wrap():
    mapped, ref, start = sam_keys(wrap_text())
    got = sort_order(*as_columns(mapped, ref, start)).tolist()
    assert got == sort_order_ref(mapped, ref, start)


def test_sort_order_unsupported_keys():
    for ref, start in ((-2, 5), (3, -1), (3, 2 ** 32 - 1), (2 ** 31 - 1 - 10000, 5)):
        with pytest.raises(_capi.BQSRError) as e:
            sort_order(np.array([R.F_MAPPED | R.F_HAS_START] * 2, np.uint32), np.array([1, ref], np.int32),
                       np.array([1, start], np.int64))
        assert e.value.status == _capi.UNSUPPORTED and e.value.read == 1
    # the largest keys that are ordered
    got = sort_order(np.array([R.F_MAPPED | R.F_HAS_START] * 3 + [0], np.uint32),
                     np.array([2 ** 31 - 2 - 10000, 0, 2 ** 31 - 2 - 10000, 0], np.int32),
                     np.array([2 ** 32 - 2, 2 ** 32 - 2, 0, 0], np.int64))
    assert got.tolist() == [1, 2, 0, 3]


# ---- errors ------------------------------------------------------------------

GOOD = rec(b"ok", 16, 2, 50)


@pytest.mark.parametrize("lines, first", [
    ([GOOD, rec(b"pos0", 16, 2, 0), GOOD], 1),                          # POS 0: start is null
    ([rec(b"star", 16, None, 7), GOOD], 0),                             # RNAME '*', non-zero FLAG without 0x4
    ([GOOD, GOOD, rec(b"nosq", 1, b"chrNope", 7)], 2),                  # RNAME not in @SQ
    ([GOOD, rec(b"u", 4, None, 0), rec(b"first", 16, None, 0), GOOD, rec(b"second", 16, 2, 0)], 2),
])
def test_sort_null_field(lines, first):
    text = HEADER + b"".join(lines)
    s = SamText(text)
    try:
        with pytest.raises(_capi.BQSRError) as e:
            s.sort()
        assert e.value.status == _capi.NULL_FIELD
        assert e.value.read == first and ("read %d " % first) in str(e.value)
        assert s.text() == text  # the parse is unchanged
        assert_same_columns(s.batch(), SamText(text).batch())
    finally:
        s.close()


def test_sort_with_pending_set_quals():
    from adam_amd.adam_save import set_quals
    from adam_amd.job import ResidentJob
    sam = SamText.read(os.path.join(GOLD, "artificial.realigned.sam"))
    job = ResidentJob(None, None, None, 0, sam=sam)
    try:
        job.step()
        p = job._ptr
        set_quals(sam, job.bh, p(job.out_qual), p(job.out_start), p(job.out_len), p(job.exc), job.n_exc, job.sp)
        with pytest.raises(_capi.BQSRError) as e:
            sam.sort()
        assert e.value.status == _capi.INVALID_ARG
        set_quals(sam)  # the text's QUAL again: nothing pending
        sam.sort()
    finally:
        job.close()
        sam.close()


# ---- state travels -----------------------------------------------------------

def stacked_text() -> bytes:
    """fragments stacked on a few positions (MarkDuplicates keeps one per
    position and strand), unmapped reads between them, out of order"""
    rnd = random.Random(11)
    return HEADER + b"".join(rec(b"s%d" % i, rnd.choice((0, 16, 16, 4)), rnd.randrange(3), 100 * (1 + rnd.randrange(3)), 20)
                             for i in range(120))


@pytest.mark.parametrize("name", ["reads12.sam", "stacked"])
def test_sort_carries_mark_duplicates(name, tmp_path):
    # reads12.sam: MarkDuplicates finds no duplicate there (the FLAG fields are
    # rewritten all the same); the stacked fragments have them
    data = stacked_text() if name == "stacked" else open(os.path.join(GOLD, name), "rb").read()
    a, b = SamText(data), SamText(data)
    try:
        n_dup = a.mark_duplicates()
        assert b.mark_duplicates() == n_dup
        assert (n_dup > 0) == (name == "stacked")
        a.sort()
        a.rewrite(None)
        b.rewrite(None)
        marked = b.text()
        if n_dup:
            assert marked != data  # (FLAG fields changed)
        assert a.text() == sorted_sam(marked) != marked
        p = tmp_path / "s.sam"
        p.write_bytes(a.text())
        assert_same_columns(a.batch(), read_sam(str(p)))
        assert int(np.count_nonzero(a.batch().flags & R.F_DUPLICATE)) == n_dup
    finally:
        a.close()
        b.close()


# ---- transform end to end ----------------------------------------------------

def bqsr_text() -> bytes:
    """synthetic reads BQSR takes (read groups, MD), in no particular order"""
    return sam_text(synth.generate(3000, (100,), 2, 5, contig_len=500_000), n_rg=2)


def e2e_inputs(tmp_path):
    fixture = open(os.path.join(GOLD, "small_realignment_targets.sam"), "rb").read()
    inputs = {"small_realignment_targets.sam": fixture, "reversed.sam": reversed_records(fixture),
              "synthetic.sam": bqsr_text()}
    paths = {}
    for name, text in inputs.items():
        p = tmp_path / name
        p.write_bytes(text)
        paths[name] = str(p)
    return paths


def rows_in_reference_order(table):
    rows = table.to_pylist()
    order = sort_order_ref([bool(r["readMapped"]) for r in rows], [r["referenceId"] for r in rows],
                           [r["start"] for r in rows])
    return [rows[i] for i in order], order


@pytest.mark.parametrize("name, moves", [("small_realignment_targets.sam", False), ("reversed.sam", True),
                                         ("synthetic.sam", True)])
def test_transform_sort_reads_sam_and_adam(name, moves, tmp_path):
    from adam_amd import parquet as P
    src = e2e_inputs(tmp_path)[name]
    plain, srt = str(tmp_path / (name + ".plain.sam")), str(tmp_path / (name + ".sorted.sam"))
    transform(src, plain, mark_duplicates=True, recalibrate=True)
    st = transform(src, srt, mark_duplicates=True, recalibrate=True, sort_reads=True)
    assert "sort" in st["phases"]
    want = sorted_sam(open(plain, "rb").read())
    assert open(srt, "rb").read() == want
    assert (want != open(plain, "rb").read()) == moves
    # ADAM output, and ADAM in -> ADAM out
    plain_a, srt_a = str(tmp_path / (name + ".plain.adam")), str(tmp_path / (name + ".sorted.adam"))
    transform(src, plain_a, mark_duplicates=True, recalibrate=True)
    transform(src, srt_a, mark_duplicates=True, recalibrate=True, sort_reads=True)
    rows, order = rows_in_reference_order(P.read_table(plain_a))
    assert P.read_table(srt_a).to_pylist() == rows
    # (the Parquet input: the same records converted, nothing run on them yet)
    pq_in = str(tmp_path / (name + ".in.adam"))
    transform(src, pq_in)
    pq_plain, pq_srt = str(tmp_path / (name + ".pq.plain.adam")), str(tmp_path / (name + ".pq.sorted.adam"))
    transform_parquet(pq_in, pq_plain, mark_duplicates=True, recalibrate=True)
    transform(pq_in, pq_srt, mark_duplicates=True, recalibrate=True, sort_reads=True)
    rows, _ = rows_in_reference_order(P.read_table(pq_plain))
    assert P.read_table(pq_srt).to_pylist() == rows


def test_transform_sort_reads12(tmp_path):
    # reads12.sam has no MD tags: BQSR raises EMPTY_TABLE with or without the
    # flag (as the reference's finalizeTable does) and no output appears;
    # MarkDuplicates + sort runs through
    src = os.path.join(GOLD, "reads12.sam")
    for sort_reads in (False, True):
        out = str(tmp_path / ("e%d.sam" % sort_reads))
        with pytest.raises(_capi.BQSRError) as e:
            transform(src, out, mark_duplicates=True, recalibrate=True, sort_reads=sort_reads)
        assert e.value.status == _capi.EMPTY_TABLE
        assert not os.path.exists(out) and not os.path.exists(out + ".partial")
    plain, srt = str(tmp_path / "plain.sam"), str(tmp_path / "sorted.sam")
    transform(src, plain, mark_duplicates=True)
    transform(src, srt, mark_duplicates=True, sort_reads=True)
    want = sorted_sam(open(plain, "rb").read())
    assert open(srt, "rb").read() == want != open(plain, "rb").read()
    from adam_amd import parquet as P
    transform(src, str(tmp_path / "plain.adam"), mark_duplicates=True)
    transform(src, str(tmp_path / "sorted.adam"), mark_duplicates=True, sort_reads=True)
    rows, _ = rows_in_reference_order(P.read_table(str(tmp_path / "plain.adam")))
    assert P.read_table(str(tmp_path / "sorted.adam")).to_pylist() == rows


def test_transform_cli_sort_reads(tmp_path):
    src = os.path.join(GOLD, "small_realignment_targets.sam")
    out = str(tmp_path / "o.sam")
    assert main([src, out, "-mark_duplicate_reads", "-recalibrate_base_qualities", "-sort_reads"]) == 0
    plain = str(tmp_path / "p.sam")
    assert main([src, plain, "-mark_duplicate_reads", "-recalibrate_base_qualities"]) == 0
    assert open(out, "rb").read() == sorted_sam(open(plain, "rb").read())
    for flag in (["-realignIndels"], ["-coalesce", "4"]):  # still refused, and the message says which
        with pytest.raises(SystemExit):
            main([src, str(tmp_path / "x.sam")] + flag)


def test_transform_sort_reads_needs_one_partition(tmp_path):
    src = tmp_path / "in.sam"
    src.write_bytes(bqsr_text())
    for out in (str(tmp_path / "o.sam"), str(tmp_path / "o.adam")):
        with pytest.raises(ValueError, match="-sort_reads needs the input in one partition; raise -partition_bytes"):
            transform(str(src), out, recalibrate=True, partition_bytes=200_000, sort_reads=True)
        assert not os.path.exists(out) and not os.path.exists(out + ".partial")
