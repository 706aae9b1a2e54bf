"""`compare` / `findreads` on the host (adam_amd/compare.py compare_host and
its building blocks): the assertions of the reference's ComparisonsSuite,
ComparisonTraversalEngineSuite, HistogramSuite and AggregatorSuite (the ones on
count, countIdentical and ++), a hand-built SAM pair per quirk, filter parsing
and the command line.  No GPU."""
import dataclasses
import io
import os
from contextlib import redirect_stdout

import pytest

from adam_amd import _capi, compare as C
from adam_amd.compare import Read

GOLD = os.path.join(os.path.dirname(__file__), "golden", "reference_resources")
HDR = b"@SQ\tSN:c\tLN:1000\n@SQ\tSN:d\tLN:1000\n@RG\tID:g\n@RG\tID:h\n"


def rec(name, flag, qual, rg=b"g", ref=b"c", pos=10, mapq=60):
    n = len(qual) if qual != b"*" else 1
    return b"%s\t%d\t%s\t%d\t%d\t%dM\t*\t0\t0\t%s\t%s\tRG:Z:%s\n" % (name, flag, ref, pos, mapq, n, b"A" * n, qual, rg)


def pair(tmp_path, body1, body2):
    p1, p2 = tmp_path / "1.sam", tmp_path / "2.sam"
    p1.write_bytes(HDR + body1)
    p2.write_bytes(HDR + body2)
    return str(p1), str(p2)


def bucket(*reads):
    bs = C.buckets_of(list(reads))
    assert len(bs) == 1
    return bs[0]


# ---- ComparisonsSuite.scala:98-123

RECORD = Read(name=b"test", dup=False, mapq=10, quals=C.quality_scores("abcdef"), reference_id=1, start=100,
              primary=True, rg="groupid", mapped=True)


def with_(**kw):
    return bucket(dataclasses.replace(RECORD, **kw))


def test_dupe_mismatches_found():
    b = with_()
    assert C.dupemismatch(b, b) == [(0, 0)]
    assert C.dupemismatch(b, with_(dup=True)) == [(0, 1)]


def test_mismatched_mapped_positions_histogram_generated():
    b = with_()
    assert C.hist_of(C.positions(b, b))[0] == 1
    moved_chr = C.hist_of(C.positions(b, with_(reference_id=2, start=200)))
    assert 0 not in moved_chr and moved_chr[-1] == 1
    moved_start = C.hist_of(C.positions(b, with_(start=200)))
    assert 0 not in moved_start and moved_start[100] == 1


def test_map_quality_scores():
    b = with_()
    assert (10, 10) in C.mapqs(b, b)
    pts = C.mapqs(b, with_(mapq=11))
    assert (10, 11) in pts or (11, 10) in pts


def test_base_quality_scores():
    b = with_()
    pts = C.baseqs(b, b)
    assert len(pts) == 6 and all(a == b_ for a, b_ in pts)


def test_unset_fields_unbox_null():
    # bucketMapqUnset / bucketQualUnset: the reference's getMapq / qualityScores on null throw
    b = with_()
    with pytest.raises(C.CompareNullField) as e:
        C.mapqs(b, with_(mapq=None))
    assert (e.value.status, e.value.side, e.value.comparison) == (_capi.NULL_FIELD, 2, "mapqs")
    with pytest.raises(C.CompareNullField) as e:
        C.baseqs(with_(quals=None), b)
    assert (e.value.side, e.value.comparison) == (1, "baseqs")


# ---- ComparisonTraversalEngineSuite.scala:27-111

def _a0(**kw):
    return dataclasses.replace(Read(rg="group0", name=b"read0", reference_id=0, start=100, primary=True, paired=False,
                                    mapped=True), **kw)


def test_generate_works_on_a_simple_rdd():
    a = [_a0(), _a0(name=b"read1", start=200, index=1)]
    b = [_a0(start=105), _a0(name=b"read1", start=200, index=1)]
    rows, _, _ = C.generate(C.buckets_of(a), C.buckets_of(b), ("positions",))
    gen = {b1.name.decode(): v["positions"] for b1, _, v in rows}
    assert len(gen) == 2
    assert "read0" in gen and "read1" in gen
    assert gen["read0"] == [5]
    assert gen["read1"] == [0]


def test_combine_works_on_a_simple_rdd():
    a = [_a0(), _a0(name=b"read1", start=200, index=1), _a0(name=b"read2", start=300, index=2)]
    b = [_a0(), _a0(name=b"read1", start=200, index=1), _a0(name=b"read2", start=305, index=2)]
    h = C.compare_reads(a, b, ("positions",)).histograms["positions"]
    assert C.hist_count(h) == 3
    assert C.hist_identical(h) == 2
    assert h[0] == 2
    assert h[5] == 1


# ---- HistogramSuite.scala:20-22, AggregatorSuite.scala:32-41

def test_histogram_addition_works():
    assert C.hist_add(C.hist_of([1]), C.hist_of([1]))[1] == 2


def test_histogram_aggregator_counts_values_correctly():
    agg = {}
    for x in (0, 0, 1):
        agg = C.hist_add(agg, C.hist_of([x]))
    assert C.hist_count(agg) == 3
    assert C.hist_identical(agg) == 2
    assert agg[0] == 2
    assert agg[1] == 1


def test_identity_keys():
    assert C.is_identical((3, 3)) and not C.is_identical((3, 4))
    assert C.is_identical(0) and not C.is_identical(-1)
    assert C.is_identical(True) and not C.is_identical(False)


# ---- one SAM pair per quirk

ALL = C.COMPARISON_NAMES


def test_flag_0_reads_count_as_unmapped(tmp_path):
    p1, p2 = pair(tmp_path, rec(b"a", 0, b"IIII"), rec(b"a", 0, b"IIIH"))
    r = C.compare_host(p1, p2, ALL)
    assert (r.total1, r.unique1, r.total2, r.unique2) == (1, 0, 1, 0)
    assert r.histograms == {"overmatched": {True: 1}, "dupemismatch": {}, "positions": {0: 1}, "mapqs": {}, "baseqs": {}}
    # FLAG 0x400 alone is a non-zero word: mapped, primary, duplicate
    p1, p2 = pair(tmp_path, rec(b"a", 0x400, b"II"), rec(b"a", 0x200, b"II"))
    assert C.compare_host(p1, p2, ["dupemismatch"]).histograms["dupemismatch"] == {(1, 0): 1}


def test_positions_minus_one_sums(tmp_path):
    # a: first of pair moved to another reference (-1), second moved by 7: the sum is 6
    # b: two categories mismatched in size: -2;  c: same place: 0
    f1 = (rec(b"a", 0x41, b"II") + rec(b"a", 0x81, b"II", pos=20) + rec(b"b", 0x41, b"II") + rec(b"b", 0x81, b"II") +
          rec(b"c", 16, b"II"))
    f2 = (rec(b"a", 0x41, b"II", ref=b"d") + rec(b"a", 0x81, b"II", pos=27) + rec(b"b", 16, b"II") +
          rec(b"c", 16, b"II"))
    p1, p2 = pair(tmp_path, f1, f2)
    r = C.compare_host(p1, p2, ["positions", "overmatched"])
    assert r.histograms["positions"] == {6: 1, -3: 1, 0: 1}
    assert r.histograms["overmatched"] == {True: 2, False: 1}


def test_unpaired_secondary_is_ignored(tmp_path):
    p1, p2 = pair(tmp_path, rec(b"a", 0x100, b"II") + rec(b"a", 0x100, b"II"), rec(b"a", 0x100, b"IH", pos=99))
    r = C.compare_host(p1, p2, ALL)
    assert r.histograms == {"overmatched": {True: 1}, "dupemismatch": {}, "positions": {0: 1}, "mapqs": {}, "baseqs": {}}


def test_same_name_cross_product_across_read_groups(tmp_path):
    f1 = rec(b"a", 16, b"I", rg=b"g") + rec(b"a", 16, b"J", rg=b"h") + rec(b"u", 16, b"I")
    f2 = rec(b"a", 16, b"K", rg=b"g") + rec(b"a", 16, b"L", rg=b"h") + rec(b"a", 16, b"M", rg=b"nohdr")
    p1, p2 = pair(tmp_path, f1, f2)
    r = C.compare_host(p1, p2, ["baseqs", "overmatched"])
    assert (r.total1, r.unique1, r.total2, r.unique2) == (3, 1, 3, 0)
    assert r.histograms["overmatched"] == {True: 6}
    assert r.histograms["baseqs"] == {(a, b): 1 for a in (40, 41) for b in (42, 43, 44)}


def test_category_of_two_reads(tmp_path):
    p1, p2 = pair(tmp_path, rec(b"a", 16, b"II") + rec(b"a", 16, b"II"), rec(b"a", 16, b"II") + rec(b"a", 16, b"II"))
    r = C.compare_host(p1, p2, ALL)
    assert r.histograms == {"overmatched": {False: 1}, "dupemismatch": {}, "positions": {-1: 1}, "mapqs": {},
                            "baseqs": {}}


def test_quals_of_unequal_length_and_star(tmp_path):
    p1, p2 = pair(tmp_path, rec(b"a", 16, b"IIII") + rec(b"s", 16, b"*"), rec(b"a", 16, b"IJ") + rec(b"s", 16, b"I"))
    r = C.compare_host(p1, p2, ["baseqs"])
    assert r.histograms["baseqs"] == {(40, 40): 1, (40, 41): 1, (9, 40): 1}


def test_utf8_side_with_2_and_3_byte_chars(tmp_path):
    s = "Ié€\U0001F600"  # 1, 2, 3 and 4 bytes; the last is a surrogate pair, two chars
    p1, p2 = pair(tmp_path, rec(b"a", 16, bytes([0x49, 0xE9, 0xAC, 0x3D, 0x00, 0x21])), rec(b"a", 16, s.encode("utf-8")))
    r = C.compare_host(p1, p2, ["baseqs"], "latin-1", "utf-8")
    sc = C.quality_scores("".join(map(chr, (0x49, 0xE9, 0xAC, 0x3D, 0x00))))
    assert r.histograms["baseqs"] == {(a, a): 1 for a in sc}  # 0xD83D, 0xDE00: low bytes 0x3D, 0x00
    assert C.hist_count(r.histograms["baseqs"]) == 5
    # 2- and 3-byte chars: the same as compare_baseqs
    p1, p2 = pair(tmp_path, rec(b"a", 16, bytes([0x49, 0xE9, 0xAC])), rec(b"a", 16, s[:3].encode("utf-8")))
    assert C.compare_host(p1, p2, ["baseqs"], "latin-1", "utf-8").histograms["baseqs"] == dict(
        C.compare_baseqs(p1, p2, "latin-1", "utf-8")["histogram"])


def test_mapq_255_raises_under_mapqs_only(tmp_path):
    f1 = rec(b"a", 16, b"II") + rec(b"b", 16, b"II", mapq=255) + rec(b"c", 16, b"II", mapq=255)
    f2 = rec(b"a", 16, b"II", mapq=255) + rec(b"b", 16, b"II") + rec(b"c", 16, b"II")
    p1, p2 = pair(tmp_path, f1, f2)
    r = C.compare_host(p1, p2, ["overmatched", "dupemismatch", "positions", "baseqs"])
    assert r.histograms["positions"] == {0: 3}
    with pytest.raises(C.CompareNullField) as e:
        C.compare_host(p1, p2, ALL)
    assert (e.value.status, e.value.comparison, e.value.side, e.value.read) == (_capi.NULL_FIELD, "mapqs", 1, 1)
    # RNAME '*' : referenceId, start and mapq are null; two null referenceIds compare equal -> start unboxes
    p1, p2 = pair(tmp_path, rec(b"x", 16, b"II") + rec(b"a", 16, b"II", ref=b"*"), rec(b"a", 16, b"II", ref=b"*"))
    with pytest.raises(C.CompareNullField) as e:
        C.compare_host(p1, p2, ["positions"])
    assert (e.value.comparison, e.value.side, e.value.read) == ("positions", 1, 1)
    assert C.compare_host(p1, p2, ["baseqs"]).histograms["baseqs"] == {(40, 40): 2}


def test_empty_join(tmp_path):
    p1, p2 = pair(tmp_path, rec(b"a", 16, b"II"), rec(b"b", 16, b"II") + rec(b"c", 16, b"II"))
    r = C.compare_host(p1, p2, ALL)
    assert (r.total1, r.unique1, r.total2, r.unique2) == (1, 1, 2, 2)
    assert all(h == {} for h in r.histograms.values())
    text = C.summary_all(p1, p2, r, ALL)
    assert text.count("count: 0") == 5 and text.count("nan") == 5


def _known_pair(tmp_path):
    f1 = (rec(b"a", 512, b"IIII") + rec(b"b", 512, b"II") + rec(b"c", 0x41, b"III") + rec(b"d", 512, b"JJ") +
          rec(b"d", 512, b"JJ") + rec(b"e", 0, b"KKKK") + rec(b"f", 0x101, b"LL"))
    f2 = (rec(b"a", 512, b"IIIH") + rec(b"c", 0x81, b"III") + rec(b"d", 512, b"JJ") + rec(b"d", 512, b"JJ") +
          rec(b"e", 0, b"KKKK") + rec(b"f", 0x181, b"LM") + rec(b"z", 512, b"I"))
    return pair(tmp_path, f1, f2)


def test_baseqs_equals_compare_baseqs(tmp_path):
    cases = [_known_pair(tmp_path) + ("latin-1", "latin-1"),
             (os.path.join(GOLD, "artificial.realigned.sam"),) * 2 + ("latin-1", "latin-1")]
    q1, q2 = tmp_path / "q1.sam", tmp_path / "q2.sam"
    q1.write_bytes(HDR + rec(b"a", 512, "Ié".encode("latin-1")))
    q2.write_bytes(HDR + rec(b"a", 512, "Ié".encode("utf-8")))
    cases.append((str(q1), str(q2), "latin-1", "utf-8"))
    for p1, p2, e1, e2 in cases:
        old = C.compare_baseqs(p1, p2, e1, e2)
        new = C.compare_host(p1, p2, ["baseqs"], e1, e2)
        assert (new.total1, new.unique1, new.total2, new.unique2) == (old["total1"], old["unique1"], old["total2"],
                                                                      old["unique2"])
        assert new.histograms["baseqs"] == dict(old["histogram"])
        assert C.summary_all(p1, p2, new, ["baseqs"]) == C.summary(p1, p2, old)


# ---- filters

def test_filter_legal_forms():
    T = C.FilterTerm
    assert C.parse_filters("overmatched=true") == [T("overmatched", "=", True)]
    assert C.parse_filters("overmatched=FALSE") == [T("overmatched", "=", False)]
    assert C.parse_filters("positions=0") == [T("positions", "=", 0)]
    assert C.parse_filters("positions>-1") == [T("positions", ">", -1)]
    assert C.parse_filters("positions<100") == [T("positions", "<", 100)]
    assert C.parse_filters("dupemismatch=(1,0)") == [T("dupemismatch", "=", (1, 0))]
    assert C.parse_filters("mapqs!=( 60 , -1 )") == [T("mapqs", "!=", (60, -1))]
    assert C.parse_filters("baseqs!=(40,40);mapqs=(60,60)") == [T("baseqs", "!=", (40, 40)), T("mapqs", "=", (60, 60))]
    assert C.combined_name(C.parse_filters("baseqs!=(40,40);mapqs=(60,60)")) == "(baseqs+mapqs)"


@pytest.mark.parametrize("text,message", [
    ("positions!=0", '"0" isn\'t a legal filter value for positions'),
    ("overmatched!=true", '"true" isn\'t a legal filter value for overmatched'),
    ("overmatched<true", '"true" isn\'t a legal filter value for overmatched'),
    ("mapqs>(1,2)", '"(1,2)" isn\'t a legal filter value for mapqs'),
    ("baseqs=40", '"40" doesn\'t match point regex'),
    ("positions=x", 'For input string: "x"'),
    ("overmatched=yes", 'For input string: "yes"'),
    ("nosuch=1", "Could not find comparison nosuch"),
    ("positions", "positions"),
    ("=3", "=3"),
])
def test_filter_refusals(text, message):
    with pytest.raises(ValueError) as e:
        C.parse_filters(text)
    assert str(e.value) == message


def test_conjunction_with_exists_per_term(tmp_path):
    # a: quals differ at one base, mapq 60 both; b: quals equal; c: differ, mapq 30 on side 2; u: unmatched
    f1 = rec(b"a", 16, b"IIII") + rec(b"b", 16, b"II") + rec(b"c", 16, b"II") + rec(b"u", 0, b"II")
    f2 = rec(b"a", 16, b"IIIH") + rec(b"b", 16, b"II") + rec(b"c", 16, b"HH", mapq=30, pos=14) + rec(b"u", 0, b"II")
    p1, p2 = pair(tmp_path, f1, f2)
    name, rows = C.find_reads_host(p1, p2, "baseqs!=(40,40);mapqs=(60,60)")
    assert name == "(baseqs+mapqs)"
    assert rows == [("a", "c:9", "c:9")]
    assert C.find_reads_host(p1, p2, "baseqs!=(40,40)")[1] == [("a", "c:9", "c:9"), ("c", "c:9", "c:13")]
    # u produced no mapq point: its term fails; overmatched produced a value for every pair
    assert [r[0] for r in C.find_reads_host(p1, p2, "overmatched=true")[1]] == ["a", "b", "c", "u"]
    assert [r[0] for r in C.find_reads_host(p1, p2, "positions>0")[1]] == ["c"]
    assert C.find_reads_host(p1, p2, "dupemismatch=(1,0)")[1] == []
    assert C.find_reads_text(name, rows) == "(baseqs+mapqs)\na\tc:9\tc:9\n"
    # allReads.head of an unmapped read without a reference prints nulls
    p1, p2 = pair(tmp_path, rec(b"n", 4, b"I", ref=b"*", pos=0), rec(b"n", 4, b"I"))
    assert C.find_reads_host(p1, p2, "overmatched=true")[1] == [("n", "null:null", "c:9")]


def test_host_path_refuses_bam_and_parquet(tmp_path, monkeypatch):
    # without a device only SAM text can be read: said so, not a parse error from the middle of a BAM
    monkeypatch.setattr(C, "_have_device", lambda: False)
    p1, p2 = pair(tmp_path, rec(b"a", 16, b"II"), rec(b"a", 16, b"II"))
    bam = tmp_path / "x.bam"
    bam.write_bytes(b"\x1f\x8b\x08\x04" + b"\0" * 20)
    adam = tmp_path / "x.adam"
    adam.mkdir()
    for a, b in ((str(bam), p2), (p1, str(adam))):
        with pytest.raises(ValueError) as e:
            C.compare(a, b, ["baseqs"])
        assert "SAM text only" in str(e.value)
        with pytest.raises(ValueError) as e:
            C.find_reads(a, b, "overmatched=true")
        assert "SAM text only" in str(e.value)
    assert C.compare(p1, p2, ["baseqs"]).histograms["baseqs"] == {(40, 40): 2}


# ---- command line

def _run(argv):
    out = io.StringIO()
    with redirect_stdout(out):
        assert C.main(argv) == 0
    return out.getvalue()


def test_cli_default_stdout_is_todays(tmp_path):
    p1, p2 = _known_pair(tmp_path)
    assert _run([p1, p2]) == C.summary(p1, p2, C.compare_baseqs(p1, p2)) + "\n"
    out = tmp_path / "h.txt"
    _run([p1, p2, "-output", str(out)])
    assert out.read_text() == "value\tcount\n(40,39)\t1\n(40,40)\t3\n(43,43)\t1\n(43,44)\t1\n"


def test_cli_output_dir(tmp_path):
    p1, p2 = _known_pair(tmp_path)
    d = tmp_path / "out"
    assert _run([p1, p2, "-comparisons", "all", "-output_dir", str(d)]) == ""
    assert sorted(os.listdir(d)) == sorted(["files", "summary.txt"] + list(ALL))
    assert (d / "files").read_text() == p1 + "\n" + p2 + "\n"
    r = C.compare_host(p1, p2, ALL)
    assert (d / "summary.txt").read_text() == C.summary_all(p1, p2, r, ALL) + "\n"
    assert (d / "overmatched").read_text() == "value\tcount\nfalse\t2\ntrue\t3\n"
    assert (d / "positions").read_text() == "value\tcount\n-2\t1\n-1\t1\n0\t3\n"
    assert (d / "mapqs").read_text() == "value\tcount\n(60,60)\t2\n"
    assert (d / "dupemismatch").read_text() == "value\tcount\n(0,0)\t2\n"
    assert (d / "baseqs").read_text() == "value\tcount\n(40,39)\t1\n(40,40)\t3\n(43,43)\t1\n(43,44)\t1\n"


def test_cli_list_comparisons_and_refusals(tmp_path, capsys):
    text = _run(["-list_comparisons"])
    assert text.startswith("\nAvailable comparisons:\n")
    assert "\t%10s : %s\n" % C.COMPARISONS[0] in text and len(text.splitlines()) == 7
    p1, p2 = _known_pair(tmp_path)
    with pytest.raises(SystemExit):
        C.main([p1, p2, "-recurse1", "x.*"])
    assert "-recurse1" in capsys.readouterr().err
    with pytest.raises(ValueError) as e:
        C.main([p1, p2, "-comparisons", "baseqs,nosuch"])
    assert str(e.value) == "Could not find comparison nosuch"
    with pytest.raises(SystemExit):
        C.main([p1, p2, "-comparisons", "all", "-output", str(tmp_path / "x")])
