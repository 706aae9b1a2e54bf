"""adam2sam's rules on the host: tests/_adam_lines_ref.py (ADAMRecord fields
-> SAM line, and the synthesised header) against tests/_adam_ref.convert_sam,
the restatement of SAMRecordConverter the ADAM columns are checked with -- a
line must come back from its own ADAMRecord.  The device's text is held to
_adam_lines_ref in tests/test_gpu_adam_lines.py."""
import glob
import os

import pytest

import _adam_lines_ref as R
from _adam_ref import convert_sam

RES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_resources")
FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(RES, "*.sam")))
# lines that do not come back byte for byte, of the file's lines -- each differs in TLEN (ADAMRecord has no field
# for it: 0 comes back) or in the order of its tags (htsjdk's order comes back, MD last), and in nothing else
DIFFERING = {"artificial.realigned.sam": (10, 10), "artificial.sam": (5, 10), "reads12.sam": (0, 200),
             "small.sam": (0, 20), "small_realignment_targets.sam": (7, 7), "unmapped.sam": (0, 200)}


def fixture(name: str) -> bytes:
    with open(os.path.join(RES, name), "rb") as fh:
        return fh.read()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_canonical_sam_comes_back_byte_for_byte(seed):
    text = R.canonical_sam(400, seed)
    recs = convert_sam(text, R.run_date)
    assert len(recs) == 400 and R.lines(recs) == R.body(text)
    # the generator reaches what it is for
    flags = {int(l.split(b"\t")[1]) for l in R.body(text).split(b"\n") if l}
    assert 0 in flags and any(f & 0x100 for f in flags) and any(f & 0x8 for f in flags) and 0x104 not in flags
    assert b"\t=\t" in text and b"\tX0:Z:\t" in text + b"\t" and b"\tXF:f:" in text


def test_fixture_names_are_the_ones_listed():
    assert FIXTURES == sorted(DIFFERING)


@pytest.mark.parametrize("name", sorted(DIFFERING))
def test_fixtures_come_back_but_for_tlen_and_tag_order(name):
    text = fixture(name)
    got = R.lines(convert_sam(text, R.run_date)).split(b"\n")[:-1]
    want = R.body(text).split(b"\n")[:-1]
    assert len(got) == len(want)
    differing = 0
    for g, w in zip(got, want):
        if g == w:
            continue
        differing += 1
        gf, wf = g.split(b"\t"), w.split(b"\t")
        assert gf[:8] == wf[:8] and gf[9:11] == wf[9:11] and gf[8] == b"0", (g, w)  # TLEN alone among the eleven
        assert sorted(gf[11:]) == sorted(wf[11:]), (g, w)  # the same tags
        md = [t for t in gf[11:] if t.startswith(b"MD:")]
        rest = [t for t in gf[11:] if not t.startswith(b"MD:")]
        assert gf[11:] == sorted(rest, key=lambda t: (t[1], t[0])) + md, g  # htsjdk's order, MD last
        assert wf[8] != b"0" or gf[11:] != wf[11:]
    assert (differing, len(want)) == DIFFERING[name]


@pytest.mark.parametrize("name", sorted(DIFFERING))
def test_synthesised_header_has_the_used_names_in_order(name):
    text = fixture(name)
    sq = [l.split(b"\t")[1][3:] for l in R.head(text).split(b"\n") if l.startswith(b"@SQ")]
    rg = [l.split(b"\t")[1][3:] for l in R.head(text).split(b"\n") if l.startswith(b"@RG")]
    used_sq, used_rg = set(), set()
    for l in R.body(text).split(b"\n")[:-1]:
        f = l.split(b"\t")
        used_sq |= {f[2], f[2] if f[6] == b"=" else f[6]} & set(sq)
        used_rg |= {t[5:] for t in f[11:] if t.startswith(b"RG:Z:")} & set(rg)
    head = R.header(convert_sam(text, R.run_date)).split(b"\n")[:-1]
    assert [l.split(b"\t")[1] for l in head if l.startswith(b"@SQ")] == [b"SN:" + n for n in sq if n in used_sq]
    assert [l.split(b"\t")[1] for l in head if l.startswith(b"@RG")] == [b"ID:" + n for n in sorted(used_rg)]
    assert all(l.startswith((b"@SQ\t", b"@RG\t")) for l in head)  # no @HD, @PG or @CO
    want_ln = {l.split(b"\t")[1][3:]: l for l in R.head(text).split(b"\n") if l.startswith(b"@SQ")}
    for l in head:
        if l.startswith(b"@SQ"):
            assert l.split(b"\t")[2] in want_ln[l.split(b"\t")[1][3:]].split(b"\t")  # its LN


def test_canonical_header_lines_and_order():
    recs = convert_sam(R.canonical_sam(300), R.run_date)
    assert R.header(recs) == (b"@SQ\tSN:chr1\tLN:250000000\n@SQ\tSN:chr2\tLN:200000000\tUR:file:/ref.fa\n"
                              b"@RG\tID:rgA\tCN:here\tDT:2013-02-03T04:05:06Z\tLB:lib1\tPI:300\tSM:s1\n"
                              b"@RG\tID:rgB\tLB:lib2\tPL:illumina\tSM:s2\n")


# ---- where the converter loses information ----

BASE = dict(readName="r", sequence="ACGT", qual="IIII", cigar="4M", attributes="")


def test_flag_0x104_comes_back_as_0():
    sam = R.HEAD + b"r\t260\tchr1\t5\t7\t*\t*\t0\t0\tACGT\tIIII\n"
    rec, = convert_sam(sam)
    assert not any(rec[k] for k in R.BOOLS)
    assert R.line(rec).split("\t")[1] == "0"
    assert R.flag_of(dict(BASE, readMapped=True, primaryAlignment=True)) == 0
    assert R.flag_of(dict(BASE, readMapped=True)) == 0x100 and R.flag_of(dict(BASE, primaryAlignment=True)) == 0x4
    assert R.flag_of(dict(BASE, mateNegativeStrand=True)) == 0x124  # 0x8 needs readPaired, 0x20 does not
    assert R.flag_of(dict(BASE, readPaired=True, readMapped=True, primaryAlignment=True)) == 0x9


def test_null_mapq_with_and_without_a_reference():
    sam = R.HEAD + b"a\t0\tchr1\t5\t255\t4M\t*\t0\t0\tACGT\tIIII\nb\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\n"
    a, b = convert_sam(sam)
    assert a["mapq"] is None and b["mapq"] is None
    assert R.lines([a, b]) == R.body(sam)
    assert R.line(dict(BASE, referenceName="chr1", mapq=0)).split("\t")[4] == "0"


def test_a_record_with_every_field_null():
    assert R.line({}) == "*\t0\t*\t0\t0\t*\t*\t0\t0\t*\t*"
    assert R.line(dict.fromkeys(list(BASE) + ["mismatchingPositions", "start", "mapq"])) == R.line({})
    assert R.header([{}]) == b""
    assert R.line(dict(mismatchingPositions="")) == R.line({}) + "\tMD:Z:"  # not null: the tag, empty


def test_run_date_round_trip():
    for ms in (0, 1359864306000, 1359864306007, 951782400000):
        assert R.run_date(R.epoch_ms_iso8601(ms)) == ms
    assert R.epoch_ms_iso8601(1359864306000) == "2013-02-03T04:05:06Z"
    assert R.epoch_ms_iso8601(1359864306007) == "2013-02-03T04:05:06.007Z"
    rec = dict(BASE, recordGroupName="g", recordGroupRunDateEpoch=1359864306000)
    assert R.header([rec]) == b"@RG\tID:g\tDT:2013-02-03T04:05:06Z\n"


def test_refusals_of_the_restatement():
    for bad in (dict(readName="a\tb"), dict(qual="I\nI"), dict(mismatchingPositions="4\r"), dict(start=-1),
                dict(mateAlignmentStart=2 ** 31 - 1), dict(mapq=256), dict(attributes="NM:i:1\nX")):
        with pytest.raises(R.Unrepresentable):
            R.line(dict(BASE, **bad))
    for bad in ("NM:i", "1M:i:3", "NM:x:3", "NM:i:1\t", "\tNM:i:1", "NM:i:1\t\tXT:A:U", "N:i:1"):
        with pytest.raises(R.Malformed):
            R.line(dict(BASE, attributes=bad))
    assert R.line(dict(BASE, start=2 ** 31 - 2, attributes="XB:B:c,1\tXH:H:1F")).endswith("\tXH:H:1F\tXB:B:c,1")
    for a, b in ((dict(referenceId=0, referenceName="x"), dict(referenceId=0, referenceName="y")),
                 (dict(referenceId=0, referenceName="x"), dict(mateReferenceId=1, mateReference="x")),
                 (dict(referenceId=0, referenceName="x", referenceLength=5),
                  dict(referenceId=0, referenceName="x", referenceLength=6)),
                 (dict(recordGroupName="g", recordGroupSample="a"), dict(recordGroupName="g", recordGroupSample="b"))):
        with pytest.raises(ValueError):
            R.header([a, b])
