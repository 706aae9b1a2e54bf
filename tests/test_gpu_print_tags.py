"""`adam print_tags` on the device (bqsr_sam_tag_counts, bqsr_arrow_tag_counts,
bqsr_sam_tag_values, bqsr_arrow_tag_values, adam_amd/csrc/tags.hip,
adam_amd/print_tags.py) against the restatement of the reference
(tests/_tags_ref.py: cli/PrintTags.scala:61-89, rdd/AdamRDDFunctions.scala:
200-229, util/AttributeUtils.scala:28-99).  Every count is compared exactly."""
import ctypes
import functools
import os

import numpy as np
import pytest

from _adam_ref import convert_sam
from _tags_ref import (TagRefError, characterize_tag_values, characterize_tags, print_tags_ref, sam_records,
                       table_records)
from adam_amd import _capi
from adam_amd import print_tags as PT
from adam_amd.bam_writer import sam_to_bam
from adam_amd.sam import SamText
from adam_amd.transform import sam_partitions

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "reference_resources")
FIXTURES = ["artificial.realigned.sam", "artificial.sam", "reads12.sam", "small.sam",
            "small_realignment_targets.sam", "unmapped.sam"]
# the wave (64) and workgroup (256) tails, more than one workgroup; the grid stride: test_grid_stride
SIZES = [1, 63, 64, 65, 255, 256, 257]
N_STRIDE = 70001
KINDS = ["same", "distinct", "mixed"]
HEADER = b"@HD\tVN:1.4\n@SQ\tSN:chr1\tLN:100000000\n"
ALPHA = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789"
STATUS = {"ATTRIBUTE": _capi.ATTRIBUTE, "NULL_FIELD": _capi.NULL_FIELD, "UNSUPPORTED": _capi.UNSUPPORTED}


# ---- inputs --------------------------------------------------------------------
# a spec is (failed, pieces): failedVendorQualityChecks and the optional fields in input order

def same_pieces(i):
    """the tag sequence of every lane the same: the leader loop runs once a step"""
    return [b"NM:i:%d" % (i % 5), b"AS:i:%d" % ((i % 3 - 1) * 100), b"XS:i:0", b"XA:Z:chr%d,+%d" % (i % 4, i % 4),
            b"MQ:f:%s" % (b"1.5" if i % 2 else b"0.25"), b"XC:A:%s" % b"ab"[i % 2:i % 2 + 1]]


def distinct_piece(i):
    """every lane of a wavefront another tag: the leader loop runs 64 times a step"""
    return b"%s:i:%d" % ((ALPHA[i % 62] + ALPHA[(i // 62) % 62]).encode(), i)


def spec(i, kind):
    if kind == "same":
        return i % 11 == 10, same_pieces(i)
    if kind == "distinct":
        return i % 13 == 12, [distinct_piece(i)]
    k = i % 6
    if k == 0:
        return False, []                                                      # no tags
    if k == 1:
        return False, [b"%sx:Z:v%d" % (ALPHA[j].encode(), j) for j in range(48)]  # 48 tags
    if k == 2:
        return False, [b"XR:i:1", b"NM:i:2", b"XR:i:%d" % (i % 4)]             # a repeated tag
    if k == 3:
        return False, same_pieces(i)
    if k == 4:
        return False, [distinct_piece(i), b"NM:i:-7"]
    return True, [b"NM:i:1", b"XR:i:5"]                                        # QC-failed


def sam_line(i, failed, pieces):
    flag = (0x200 | 0x10) if failed else (0, 0x10, 0x1 | 0x40)[i % 3]
    return b"q%d\t%d\tchr1\t%d\t60\t4M\t*\t0\t0\tACGT\tIIII%s\n" % (i, flag, 1 + i % 977,
                                                                     b"".join(b"\t" + p for p in pieces))


def sam_text(specs):
    return HEADER + b"".join(sam_line(i, f, p) for i, (f, p) in enumerate(specs))


def arrow_records(specs):
    return [(b"\t".join(p), f) for f, p in specs]


def table(records, cuts=()):
    """an Arrow table of (attributes, failed) records; cuts: record batches of these lengths
    (sliced arrays, offsets not 0), then the rest.  The bytes need not be UTF-8."""
    import pyarrow as pa
    b = pa.array([a for a, _ in records], pa.binary())
    t = pa.table({"attributes": pa.Array.from_buffers(pa.string(), len(b), b.buffers(), null_count=b.null_count),
                  "failedVendorQualityChecks": pa.array([f for _, f in records], pa.bool_())})
    if not cuts:
        return t
    batches, a = [], 0
    for c in list(cuts) + [len(records)]:
        c = min(c, len(records) - a)
        if c > 0:
            batches += t.slice(a, c).to_batches()
            a += c
    return pa.Table.from_batches(batches)


CUTS = (1, 63, 130, 77)  # chunk lengths that are no multiples of 64


@functools.lru_cache(maxsize=None)
def generated(n, kind):
    """(SAM text, the converter's records, Arrow records); computed once"""
    specs = [spec(i, kind) for i in range(n)]
    text = sam_text(specs)
    return text, sam_records(convert_sam(text)), arrow_records(specs)


@functools.lru_cache(maxsize=None)
def wanted(n, kind):
    """the restatement's (tags, total) for the SAM and for the Arrow form"""
    _, srecs, arecs = generated(n, kind)
    return characterize_tags(srecs), characterize_tags(arecs)


def value_tags(kind):
    return {"same": ("NM", "XA", "MQ", "XC"), "distinct": ("AA", "NM"), "mixed": ("NM", "XR", "Ax", "AA")}[kind]


def sam_counts(data, bam=False):
    s = SamText(data, bam=bam)
    try:
        return s.tag_counts()
    finally:
        s.close()


def sam_values(data, tag, bits=64, bam=False):
    s = SamText(data, bam=bam)
    try:
        return s.tag_values(tag, hash_bits=bits)
    finally:
        s.close()


def arrow_counts(t):
    chunks, keep = PT.table_chunks(t)
    return PT.arrow_tag_counts(chunks)


def arrow_values(t, tag, bits=64):
    chunks, keep = PT.table_chunks(t)
    PT.arrow_tag_counts(chunks)  # (validates)
    return PT.arrow_tag_values(chunks, tag, hash_bits=bits)


def raises(status, read, fn, *args, **kw):
    with pytest.raises(_capi.BQSRError) as e:
        fn(*args, **kw)
    assert (e.value.name, e.value.read) == (status, read), str(e.value)
    assert e.value.status == STATUS.get(status, e.value.status)
    return e.value


# ---- fixtures ------------------------------------------------------------------

@pytest.mark.parametrize("name", FIXTURES)
def test_reference_fixtures(name):
    data = open(os.path.join(GOLD, name), "rb").read()
    recs = sam_records(convert_sam(data))
    want = characterize_tags(recs)
    assert want[1] > 0
    bam = sam_to_bam(data)
    assert sam_counts(data) == want
    assert sam_counts(bam, bam=True) == want
    for tag in want[0]:
        v = characterize_tag_values(recs, tag)
        assert sum(v.values()) == want[0][tag]  # (the converter leaves one attribute a tag)
        for bits in (64, 4):
            assert sam_values(data, tag, bits) == v, (tag, bits)
        assert sam_values(bam, tag, bam=True) == v, tag
    if name == "reads12.sam":  # AdamRDDFunctionsSuite.scala:539-547
        assert [want[0][t] for t in ("NM", "AS", "XS")] == [200, 200, 200]


# ---- sizes and tag patterns ----------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_generated(n, kind, tmp_path):
    text, srecs, arecs = generated(n, kind)
    swant, awant = wanted(n, kind)
    if kind == "mixed" and n >= 64:
        assert awant[0]["XR"] == 2 * swant[0]["XR"] > 0  # Arrow counts a repeated tag twice, the converter keeps one
        assert swant[1] < n  # QC-failed records
    assert sam_counts(text) == swant
    assert arrow_counts(table(arecs)) == awant
    assert arrow_counts(table(arecs, CUTS)) == awant
    for tag in value_tags(kind):
        sv, av = characterize_tag_values(srecs, tag), characterize_tag_values(arecs, tag)
        for bits in (64, 4):
            assert sam_values(text, tag, bits) == sv, (tag, bits)
            assert arrow_values(table(arecs, CUTS), tag, bits) == av, (tag, bits)
    # the same through the file entry point, in one partition and in several
    p = tmp_path / "in.sam"
    p.write_bytes(text)
    assert PT.characterize_tags(str(p)) == swant[0]
    part = max(1, (len(text) - len(HEADER)) // 6)
    assert len(sam_partitions(text, part)[1]) >= (5 if n >= 63 else 1)
    assert PT.characterize_tags(str(p), partition_bytes=part) == swant[0]
    tag = value_tags(kind)[0]
    assert PT.characterize_tag_values(str(p), tag, partition_bytes=part) == characterize_tag_values(srecs, tag)


def test_repeated_tag_value():
    """SAM keeps the last value of a repeated tag, Arrow takes the first"""
    text, srecs, arecs = generated(257, "mixed")
    sv, av = characterize_tag_values(srecs, "XR"), characterize_tag_values(arecs, "XR")
    assert av == {("i", "1"): sum(av.values())} and set(sv) == {("i", "0"), ("i", "2")}  # (i % 6 == 2: i % 4 is 0 or 2)
    assert sam_values(text, "XR") == sv
    assert arrow_values(table(arecs), "XR") == av


# BQSR_TUNE_FLAGSTAT_GRID caps the scan kernels' grids too: with one workgroup
# (4 waves) the 70 001 records take every wavefront through 273 or 274 passes
# of the grid-stride loop, with three workgroups through 91 or 92.
@pytest.mark.parametrize("grid", [0, 1, 3])
def test_grid_stride(grid):
    from adam_amd import bqsr
    text, srecs, arecs = generated(N_STRIDE, "mixed")
    swant, awant = wanted(N_STRIDE, "mixed")
    with bqsr.Context.get(0).tuned(flagstat_grid=grid):
        assert sam_counts(text) == swant
        assert arrow_counts(table(arecs, CUTS)) == awant


def test_rare_tag_bytes():
    """tag bytes outside 0x20..0x7E go straight to the global table"""
    rare = [b" ~:i:1", b"~ :A:x", b"\x01\x7f:Z:v", b"\x7f\x01:i:2", b"\x1fA:i:3", b"A\x1f:i:4", b"  :i:5", b"~~:i:6"]
    specs = [(i % 9 == 8, [rare[i % 8], rare[(i + 3) % 8], b"NM:i:1"]) for i in range(300)]
    arecs = arrow_records(specs)
    want = characterize_tags(arecs)
    assert len(want[0]) == 9 and want[0]["\x01\x7f"] > 0
    assert arrow_counts(table(arecs, CUTS)) == want
    text = sam_text(specs)
    swant = characterize_tags(sam_records(convert_sam(text)))
    assert swant == want  # (no tag repeats within a record)
    assert sam_counts(text) == swant
    assert sam_values(text, "\x01\x7f") == characterize_tag_values(arecs, "\x01\x7f") == \
        arrow_values(table(arecs), "\x01\x7f")


# ---- the filter ----------------------------------------------------------------

def test_failed_records_are_not_parsed_in_arrow():
    good = (b"NM:i:1", False)
    recs = [good] * 70 + [(b"XT:i", True), (None, True), (b"X\xc3\xa9:Z:v", True), (b"XT:B:c,1", True)] + [good] * 5
    assert arrow_counts(table(recs, CUTS)) == characterize_tags(recs) == ({"NM": 75}, 75)
    assert arrow_values(table(recs), "XT") == {}


def test_failed_record_is_converted_in_sam():
    """every record goes through SAMRecordConverter: an H tag fails the call
    as bqsr_sam_adam_prepare does, also on a QC-failed record"""
    from adam_amd.adam_save import adam_table, header_info
    specs = [(False, [b"NM:i:1"])] * 70 + [(True, [b"XH:H:1A"])] + [(False, [b"NM:i:1"])] * 5
    text = sam_text(specs)
    e = raises("UNSUPPORTED", 70, sam_counts, text)
    s = SamText(text)
    try:
        with pytest.raises(_capi.BQSRError) as a:
            adam_table(s, 0, len(specs), header_info(s))
    finally:
        s.close()
    assert (a.value.status, a.value.read, str(a.value)) == (e.status, e.read, str(e))


# ---- errors ----------------------------------------------------------------------

ERRORS = [
    (b"XT:i", "ATTRIBUTE"),             # no value
    (b"X:i:1", "ATTRIBUTE"),            # a one-char tag
    (b"X::Z:v", "ATTRIBUTE"),           # a tag containing ':'
    (b"XT:x:1", "ATTRIBUTE"),           # a type letter outside AifZHB
    (b"XT:A:", "ATTRIBUTE"),            # an empty A
    (b"XT:i:1x", "ATTRIBUTE"),
    (b"XT:i:2147483648", "ATTRIBUTE"),
    (b"XT:f:abc", "ATTRIBUTE"),
    (b"XT:H:1A", "ATTRIBUTE"),
    (b"XT:B:c,1,2", "ATTRIBUTE"),
    (b"XT:Z:a\nb", "ATTRIBUTE"),
    (b"XT:Z:a\xc2\x85b", "ATTRIBUTE"),  # U+0085
    (b"X\xc3\xa9:Z:v", "UNSUPPORTED"),  # a non-ASCII tag byte
    (b"XT:i:\xd9\xa1", "UNSUPPORTED"),  # a non-ASCII digit
]
GOOD = (b"NM:i:1\tXT:B:1,2.5\tXA:Z:\xc3\xa9\x85", False)  # (a B array and any bytes in a Z value count without error)


def with_bad(bad, at, n=90):
    recs = [GOOD] * n
    for piece, i in zip(bad, at):
        recs[i] = (b"NM:i:1\t" + piece + b"\tAS:i:2", False)  # the bad piece between two good ones
    return recs


@pytest.mark.parametrize("piece,status", ERRORS)
def test_arrow_errors(piece, status):
    recs = with_bad([piece], [70])
    with pytest.raises(TagRefError) as r:
        characterize_tags(recs)
    assert (r.value.status, r.value.read) == (status, 70)
    raises(status, 70, arrow_counts, table(recs))
    raises(status, 70, arrow_counts, table(recs, (33, 20, 10)))  # in the fourth chunk


def test_arrow_first_error_wins():
    for (p1, s1), (p2, s2) in ((ERRORS[0], ERRORS[12]), (ERRORS[12], ERRORS[0]), (ERRORS[4], ERRORS[13])):
        recs = with_bad([p1, p2], [40, 75])
        raises(s1, 40, arrow_counts, table(recs, (33, 20, 10)))
        recs[40] = (b"", None)  # a null failedVendorQualityChecks comes first
        raises("NULL_FIELD", 40, arrow_counts, table(recs, (33, 20, 10)))
    # within a record: the first bad attribute in string order
    raises("UNSUPPORTED", 0, arrow_counts, table([(b"X\xc3\xa9:Z:v\tXT:i", False)]))
    raises("ATTRIBUTE", 0, arrow_counts, table([(b"XT:i\tX\xc3\xa9:Z:v", False)]))


def test_arrow_null_fields():
    recs = [GOOD] * 90
    recs[70] = (GOOD[0], None)
    raises("NULL_FIELD", 70, arrow_counts, table(recs, (33, 20, 10)))
    recs[70] = (None, False)
    raises("NULL_FIELD", 70, arrow_counts, table(recs, (33, 20, 10)))
    with pytest.raises(TagRefError) as r:
        characterize_tags(recs)
    assert (r.value.status, r.value.read) == ("NULL_FIELD", 70)
    # an absent column is a column of nulls
    raises("NULL_FIELD", 0, arrow_counts, table([GOOD] * 90).drop(["failedVendorQualityChecks"]))
    raises("NULL_FIELD", 0, arrow_counts, table([GOOD] * 90).drop(["attributes"]))
    failed_only = table([(None, True)] * 90).drop(["attributes"])
    assert arrow_counts(failed_only) == ({}, 0)


SAM_ERRORS = [
    ([b"X::Z:v"], "ATTRIBUTE"),
    ([b"XT:A:"], "ATTRIBUTE"),
    ([b"XT:Z:a\xc2\x85b"], "ATTRIBUTE"),
    ([b"XT:Z:a\xe2\x80\xa9"], "ATTRIBUTE"),   # U+2029
    ([b"\xc3\xa9:Z:v"], "UNSUPPORTED"),       # two tag bytes >= 0x80 (one char for Java)
    ([b"X\xc3\xa9:Z:v"], "SAM_PARSE"),          # no ':' behind two bytes: the converter's error
    ([b"XT:H:1A"], "UNSUPPORTED"),            # the converter's errors, as bqsr_sam_adam_prepare reports them
    ([b"XT:B:c,1,2"], "UNSUPPORTED"),
    ([b"XT:i:2147483648"], "UNSUPPORTED"),
    ([b"XT:i:1x"], "SAM_PARSE"),
    ([b"XT:f:abc"], "SAM_PARSE"),
    ([b"%sy:i:1" % ALPHA[j].encode() for j in range(49)], "UNSUPPORTED"),  # more than 48 tags
]


@pytest.mark.parametrize("pieces,status", SAM_ERRORS)
def test_sam_errors(pieces, status, tmp_path):
    specs = [(False, [b"NM:i:1"])] * 90
    specs[70] = (False, [b"NM:i:1"] + pieces)
    specs[80] = (False, [b"XT:A:"])  # a later failing record does not matter
    text = sam_text(specs)
    raises(status, 70, sam_counts, text)
    # from a later partition: the ordinal in the whole input
    p = tmp_path / "in.sam"
    p.write_bytes(text)
    part = (len(text) - len(HEADER)) // 6
    assert len(sam_partitions(text, part)[1]) >= 5
    e = raises(status, 70, PT.characterize_tags, str(p), partition_bytes=part)
    assert "read 70" in str(e)


def test_sam_first_error_wins():
    specs = [(False, [b"NM:i:1"])] * 300
    specs[200] = (False, [b"XT:A:"])
    specs[130] = (False, [b"\xc3\xa9:Z:v"])
    raises("UNSUPPORTED", 130, sam_counts, sam_text(specs))
    specs[66] = (False, [b"XT:Z:\xc2\x85"])
    raises("ATTRIBUTE", 66, sam_counts, sam_text(specs))
    # a conversion error comes before a bad attribute of the same record, wherever it stands
    specs[66] = (False, [b"AA:A:", b"ZZ:H:00"])
    raises("UNSUPPORTED", 66, sam_counts, sam_text(specs))
    specs[66] = (True, [b"AA:A:"])  # QC-failed: converted, not parsed
    raises("UNSUPPORTED", 130, sam_counts, sam_text(specs))


# ---- values ------------------------------------------------------------------------

def both_values(specs, tag, srecs=None):
    """the values of tag over the SAM and the Arrow form, at both hash widths, against the restatement"""
    arecs = arrow_records(specs)
    text = sam_text(specs)
    if srecs is None:
        srecs = sam_records(convert_sam(text))
    sv, av = characterize_tag_values(srecs, tag), characterize_tag_values(arecs, tag)
    for bits in (64, 4):
        assert sam_values(text, tag, bits) == sv, bits
        assert arrow_values(table(arecs, CUTS), tag, bits) == av, bits
    return sv, av


def test_values_all_distinct():
    n = 1000
    specs = [(i % 10 == 9, [b"XD:Z:v%d" % i, b"XI:i:%d" % (i - 500), b"XF:f:%d.5" % i]) for i in range(n)]
    for tag in ("XD", "XI", "XF"):
        sv, av = both_values(specs, tag)
        assert sv == av and len(sv) == 900 and set(sv.values()) == {1}


def test_values_three_over_many_records():
    vals = (b"a", b"bb", b"a\tXV:Z:ccc")  # (the third: a repeat -- Arrow takes "a", SAM "ccc")
    specs = [(i % 7 == 6, [b"XV:Z:" + vals[i % 3]]) for i in range(N_STRIDE)]
    # the converter prints a single Z tag as it stands
    srecs = [((b"XV:Z:" + (b"ccc" if i % 3 == 2 else vals[i % 3])), f) for i, (f, _) in enumerate(specs)]
    sv, av = both_values(specs, "XV", srecs)
    assert len(sv) == 3 and len(av) == 2 and sum(sv.values()) == sum(av.values()) == N_STRIDE - N_STRIDE // 7


def test_values_mixed_types_under_one_tag():
    pieces = [b"XM:i:3", b"XM:Z:3", b"XM:A:3", b"XM:f:3", b"XM:i:03", b"XM:f:3.0", b"XM:f:-0.0", b"XM:f:0.0",
              b"XM:f:NaN", b"XM:f:1e10", b"XM:Z:", b"XM:A:3x", b"XM:i:-2147483648", b"XM:f:1e39", b"XM:f:-1e-46"]
    specs = [(False, [pieces[i % len(pieces)]]) for i in range(200)]
    with np.errstate(over="ignore"):  # (1e39 becomes Infinity, as Float.valueOf makes it)
        sv, av = both_values(specs, "XM")
    assert sv == av and len(sv) == 11
    assert {k for k in sv if k[1] == "3"} == {("i", "3"), ("Z", "3"), ("A", "3")}
    assert {("f", "0.0"), ("f", "-0.0"), ("f", "NaN"), ("f", "1.0E10"), ("f", "Infinity")} <= set(sv)
    # H only reaches the values through Arrow input
    arecs = [(p, False) for p in (b"XM:H:0190", b"XM:H:", b"XM:H:0190", b"XM:Z:0190", b"XM:i:190")] * 30
    want = characterize_tag_values(arecs, "XM")
    assert want[("H", "Vector(0, 1, 9, 0)")] == 60 and want[("H", "Vector()")] == 30
    for bits in (64, 4):
        assert arrow_values(table(arecs, CUTS), "XM", bits) == want


def test_runs_name_their_first_read():
    """a run's first record, global over the chunks, at both hash widths (at 4 bits "a" .. "e" share keys or not,
    and a value's runs may split: the smallest first read of its runs is the value's)"""
    from adam_amd import bqsr
    vals = [b"a", b"b", None, b"a", b"c", b"b", b"d", None, b"e", b"a"]  # None: a QC-failed record
    recs = [((b"XV:Z:" + v) if v else b"XV:Z:zz", v is None) for v in vals] * 30
    want = {}
    for i, v in enumerate(vals * 30):
        if v is not None:
            want.setdefault(("Z", v.decode()), i)
    chunks, keep = PT.table_chunks(table(recs, (7, 64, 100)))
    arr = (PT.TagsChunk * len(chunks))(*chunks)
    for bits in (64, 4, 1):
        sz = PT._ValueSizes()
        _capi.check(PT._lib().bqsr_arrow_tag_values(bqsr.Context.get(0).handle, arr, len(chunks), b"XV", bits, None,
                                                    ctypes.byref(sz)))
        counts, firsts = PT._fetch_runs(sz)
        assert firsts == want, bits
        assert counts == characterize_tag_values(recs, "XV"), bits
    # over a parse
    text = sam_text([(f, [a]) for a, f in recs])
    st = SamText(text)
    try:
        st.tag_counts()
        for bits in (64, 4):
            sz = PT._ValueSizes()
            _capi.check(PT._lib().bqsr_sam_tag_values(st.ctx.handle, st.h, b"XV", bits, None, ctypes.byref(sz)))
            assert PT._fetch_runs(sz)[1] == want, bits
    finally:
        st.close()


def test_values_of_type_b_are_unsupported():
    recs = [GOOD] * 90
    assert arrow_counts(table(recs)) == characterize_tags(recs) == ({"NM": 90, "XT": 90, "XA": 90}, 90)
    raises("UNSUPPORTED", 0, arrow_values, table(recs), "XT")
    recs = [(b"XT:i:1", False)] * 70 + [(b"XT:B:1,2.5", False)] * 5
    raises("UNSUPPORTED", 70, arrow_values, table(recs, (33, 20, 10)), "XT")
    with pytest.raises(TagRefError) as r:
        characterize_tag_values(recs, "XT")
    assert (r.value.status, r.value.read) == ("UNSUPPORTED", 70)
    recs[70:] = [(b"XT:B:1,2.5", True)] * 5  # QC-failed: not looked at
    assert arrow_values(table(recs), "XT") == {("i", "1"): 70}


def test_tag_name_length():
    text = generated(63, "same")[0]
    s = SamText(text)
    try:
        for t in ("", "N", "NMX"):
            with pytest.raises(ValueError):
                s.tag_values(t)
    finally:
        s.close()


# ---- the output ------------------------------------------------------------------------

COUNT = ("NM", "XX", "toolong")


@pytest.mark.parametrize("kind", ["sam", "bam", "parquet"])
def test_print_tags_text(kind, tmp_path, capsys):
    import pyarrow.parquet as pq
    text, srecs, arecs = generated(257, "mixed")
    recs = srecs
    path = tmp_path / "in.sam"
    if kind == "sam":
        path.write_bytes(text)
    elif kind == "bam":
        path = tmp_path / "in.bam"
        path.write_bytes(sam_to_bam(text))
    else:
        path = tmp_path / "in.parquet"
        pq.write_table(table(arecs), str(path), row_group_size=100)
        recs = table_records(pq.read_table(str(path)))
        assert recs == arecs
    want = print_tags_ref(recs, list_n=3, count=COUNT)
    assert want.count("\n") > 60 and "\n NM\t" in want and "\n\t" in want
    assert PT.print_tags(str(path), list_n=3, count=COUNT) == want
    if kind == "sam":
        assert PT.print_tags(str(path), list_n=3, count=COUNT, partition_bytes=4000) == want
        # more listed records than the first partitions hold
        assert PT.print_tags(str(path), list_n=200, partition_bytes=4000) == print_tags_ref(recs, list_n=200)
    assert PT.print_tags(str(path), list_n=0) == print_tags_ref(recs, list_n=0) == print_tags_ref(recs)
    capsys.readouterr()
    assert PT.main([str(path), "-list", "3", "-count", ",".join(COUNT)]) == 0
    cap = capsys.readouterr()
    assert cap.out == want + "\n"
    assert cap.err.startswith("reads=257 ") and "phases=" in cap.err


def test_nothing_is_printed_when_the_job_raises(tmp_path, capsys):
    specs = [(False, [b"NM:i:1"])] * 90
    specs[70] = (False, [b"XT:A:"])
    p = tmp_path / "in.sam"
    p.write_bytes(sam_text(specs))
    capsys.readouterr()
    raises("ATTRIBUTE", 70, PT.main, [str(p), "-list", "5", "-count", "NM"])
    assert capsys.readouterr().out == ""


def test_reads12_command(capsys):
    path = os.path.join(GOLD, "reads12.sam")
    assert PT.main([path, "-count", "NM"]) == 0
    out = capsys.readouterr().out.split("\n")
    recs = sam_records(convert_sam(open(path, "rb").read()))
    assert "\n".join(out) == print_tags_ref(recs, count=("NM",)) + "\n"
    assert " AS\t200" in out and " XS\t200" in out and out[-2] == "Total: 200"
    i = out.index(" NM\t200")
    values = [l for l in out[i + 1:out.index(" XS\t200")] if l.startswith("\t")]
    assert values and sum(int(l.split("\t")[1]) for l in values) == 200
