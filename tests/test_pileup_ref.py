"""The reads2ref restatement (tests/_pileup_ref.py) against the reference's own
PileupConversionSuite, hand-written rows per CIGAR operator, every throwing
kind, and the golden SAMs.  No device."""
import os

import pytest

import _adam_ref
import _pileup_ref as PR

RES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_resources")


def _suite_record(md):
    quals = [30, 20, 40, 20, 10]
    return quals, dict(start=1, mapq=30, sequence="ACTAG", cigar="5M", mismatchingPositions=md,
                       qual="".join(chr(q + 33) for q in quals), readMapped=True)


def _suite_common(pileups, quals):
    by_pos = sorted(pileups, key=lambda p: p["position"])
    assert len(pileups) == 5
    assert "".join(p["readBase"] for p in by_pos) == "ACTAG"
    assert [p["sangerQuality"] for p in by_pos] == quals
    assert all(p["mapQuality"] == 30 for p in pileups)
    assert all(p["readStart"] == 1 for p in pileups)
    assert all(p["readEnd"] == 6 for p in pileups)
    assert all(p["countAtPosition"] == 1 for p in pileups)
    assert all(p["numReverseStrand"] == 0 for p in pileups)
    assert all(p["numSoftClipped"] == 0 for p in pileups)
    assert all(p["rangeLength"] is None for p in pileups)


def test_suite_single_read_with_only_matches():
    """PileupConversionSuite "can convert a single read with only matches" """
    quals, rec = _suite_record("5")
    pileups = PR.read_to_pileups(rec)
    _suite_common(pileups, quals)
    assert all(p["readBase"] == p["referenceBase"] for p in pileups)


def test_suite_single_read_with_matches_and_mismatches():
    """PileupConversionSuite "can convert a single read with matches and mismatches" """
    quals, rec = _suite_record("4A0")
    pileups = PR.read_to_pileups(rec)
    _suite_common(pileups, quals)
    assert all(p["readBase"] == p["referenceBase"] for p in pileups if p["position"] < 5)
    assert all(p["readBase"] != p["referenceBase"] for p in pileups if p["position"] == 5)
    assert all(p["referenceBase"] == "A" for p in pileups if p["position"] == 5)
    assert [p["position"] for p in pileups] == [5, 4, 3, 2, 1]  # prepended


def _rec(cigar, md, seq, qual=None, start=100, **kw):
    r = dict(start=start, mapq=7, sequence=seq, cigar=cigar, mismatchingPositions=md,
             qual=qual if qual is not None else "".join(chr(40 + i) for i in range(len(seq or ""))),
             readMapped=True, readNegativeStrand=False, readName="r", referenceName="c", referenceId=0)
    r.update(kw)
    return r


def test_every_operator_rows_literal():
    # 2S3M2I2M3D2M: read ACGTACGTACG (11 bases), quals '(' + i; MD: 3 matches, reference C at the 4th M base, a match, ^ACG, 2 matches
    rec = _rec("2S3M2I2M3D2M", "3C1^ACG2", "ACGTACGTACG", readNegativeStrand=True)
    rows = PR.read_to_pileups(rec)
    # (position, rangeOffset, rangeLength, referenceBase, readBase, sangerQuality, numSoftClipped), walk order
    walk = [
        (100, 0, 2, None, "A", 7, 1), (100, 1, 2, None, "C", 8, 1),        # 2S at the unchanged position
        (100, None, None, "G", "G", 9, 0), (101, None, None, "T", "T", 10, 0), (102, None, None, "A", "A", 11, 0),
        (103, 0, 2, None, "C", 12, 0), (103, 1, 2, None, "G", 13, 0),      # 2I
        (103, None, None, "C", "T", 14, 0), (104, None, None, "A", "A", 15, 0),
        (105, 0, 3, "A", None, 16, 0), (106, 1, 3, "C", None, 16, 0), (107, 2, 3, "G", None, 16, 0),  # 3D: next base's qual
        (108, None, None, "C", "C", 16, 0), (109, None, None, "G", "G", 17, 0),
    ]
    got = [(r["position"], r["rangeOffset"], r["rangeLength"], r["referenceBase"], r["readBase"], r["sangerQuality"],
            r["numSoftClipped"]) for r in rows]
    assert got == walk[::-1]
    assert all(r["numReverseStrand"] == 1 and r["readStart"] == 100 and r["readEnd"] == 110 and
               r["mapQuality"] == 7 and r["readName"] == "r" and r["countAtPosition"] == 1 for r in rows)


def test_mismatch_base_comes_from_md_upper_cased():
    rows = PR.read_to_pileups(_rec("3M", "1k1", "ACG"))
    assert [(r["position"], r["referenceBase"], r["readBase"]) for r in rows] == [
        (102, "G", "G"), (101, "K", "C"), (100, "A", "A")]


def test_skips_and_other_operators():
    # N, =, X, H, P give nothing; = and X consume read and reference, N reference; the MD is looked up at
    # referencePos - start, N included (the reference's misplacement)
    rows = PR.read_to_pileups(_rec("2H1M3N1M2=1X1P1M", "9", "ACGTAC"))
    assert [(r["position"], r["readBase"]) for r in rows] == [(108, "C"), (104, "C"), (100, "A")]
    assert rows[0]["readEnd"] == 109
    # after an N the MD has ended: the M base there has neither match nor mismatch
    with pytest.raises(PR.PileupThrow) as e:
        PR.read_to_pileups(_rec("1M3N1M", "2", "AC"))
    assert e.value.status == "PILEUP"


def test_sanger_quality_wraps_as_a_signed_byte():
    rows = PR.read_to_pileups(_rec("3M", "3", "ACG", qual="~\xa1\xff"))
    assert [r["sangerQuality"] for r in rows][::-1] == [93, -128, -34]


def test_no_pileups_without_cigar_or_md():
    assert PR.read_to_pileups(_rec(None, "3", "ACG")) == []
    assert PR.read_to_pileups(_rec("3M", None, "ACG")) == []
    assert PR.read_to_pileups(_rec(None, None, "ACG", start=None)) == []
    assert PR.read_to_pileups(_rec("*", "", "ACG")) == []
    assert PR.read_to_pileups(_rec("3N2H", "", "ACG", readMapped=False)) == []


THROWS = [
    ("null start", _rec("*", "", "A", start=None), "NULL_FIELD"),
    ("null start before a bad MD", _rec("1M", "A", "A", start=None), "NULL_FIELD"),
    ("MD without a leading digit", _rec("1M", "A1", "A"), "MD_PARSE"),
    ("MD caret without bases", _rec("1M", "1^1", "A"), "MD_PARSE"),
    ("MD without a trailing digit", _rec("*", "1A", "A"), "MD_PARSE"),
    ("MD number beyond Int", _rec("1M", "2147483648", "A"), "MD_PARSE"),
    ("MD parse before the walk's faults", _rec("1M", "x", "*", readMapped=False), "MD_PARSE"),
    ("sequence *", _rec("1M", "1", "*", qual="*"), "PILEUP"),
    ("sequence =", _rec("2M", "2", "A=", qual="II"), "PILEUP"),
    ("sequence .", _rec("1S1M", "1", ".A"), "PILEUP"),
    ("lower-case sequence base", _rec("2M", "2", "Ac"), "PILEUP"),
    ("lower-case inserted base", _rec("1M1I1M", "2", "AcG"), "PILEUP"),
    ("sequence shorter than M", _rec("3M", "3", "AC", qual="III"), "PILEUP"),
    ("sequence shorter than I", _rec("1M2I", "1", "AC", qual="III"), "PILEUP"),
    ("sequence shorter than a zero-length I", _rec("1M3=0I", "4", "AC", qual="III"), "PILEUP"),
    ("sequence shorter than S", _rec("3S", "", "AC", qual="III"), "PILEUP"),
    ("quals shorter than the CIGAR", _rec("3M", "3", "ACG", qual="II"), "PILEUP"),
    ("M where the MD has a delete", _rec("2M", "1^A0", "AC"), "PILEUP"),
    ("M beyond the MD", _rec("3M", "2", "ACG"), "PILEUP"),
    ("D where the MD has a match", _rec("1M1D1M", "3", "AC"), "PILEUP"),
    ("D where the MD has a mismatch", _rec("1M1D1M", "1A1", "AC"), "PILEUP"),
    ("trailing D indexes past the quals", _rec("2M1D", "2^A0", "AC"), "PILEUP"),
    ("unmapped read with a pileup", _rec("1M", "1", "A", readMapped=False), "PILEUP"),
    ("null sequence on a match", _rec("1M", "1", None, qual="I"), "NULL_FIELD"),
    ("null sequence on an insert", _rec("1I", "", None, qual="I"), "NULL_FIELD"),
    ("null qual", _rec("1M", "1", "A", qual=None) | {"qual": None}, "NULL_FIELD"),
    # several faults in one read: the one evaluated first decides
    ("unmapped before null qual", _rec("1M", "1", "A", readMapped=False) | {"qual": None}, "PILEUP"),
    ("mismatch lookup before null sequence", _rec("1M", "0A0", None, qual="I"), "NULL_FIELD"),
    ("no MD entry before null sequence", _rec("1M", "", None, qual="I"), "PILEUP"),
    ("bad base before unmapped", _rec("1M", "1", "a", readMapped=False), "PILEUP"),
    ("null sequence (match) before unmapped", _rec("1M", "1", None, qual="I", readMapped=False), "NULL_FIELD"),
    ("D: no delete before null qual", _rec("1D", "1", "A") | {"qual": None}, "PILEUP"),
]


@pytest.mark.parametrize("name,rec,status", THROWS, ids=[t[0] for t in THROWS])
def test_throwing_kinds(name, rec, status):
    with pytest.raises(PR.PileupThrow) as e:
        PR.read_to_pileups(rec)
    assert e.value.status == status


def test_flag_zero_sam_record_throws():
    # quirk Q2: FLAG 0 leaves readMapped false; SAM input is not filtered
    sam = b"@SQ\tSN:c\tLN:1000\nr\t0\tc\t5\t30\t2M\t*\t0\t0\tAC\tII\tMD:Z:2\n"
    recs = _adam_ref.convert_sam(sam)
    assert recs[0]["readMapped"] is False
    with pytest.raises(PR.PileupThrow) as e:
        PR.reads_to_pileups(recs)
    assert (e.value.status, e.value.read) == ("PILEUP", 0)


def test_first_throwing_read_in_input_order():
    good = _rec("1M", "1", "A")
    with pytest.raises(PR.PileupThrow) as e:
        PR.reads_to_pileups([good, good, _rec("1M", "A", "A"), _rec("1M", "1", "a")])
    assert (e.value.status, e.value.read) == ("MD_PARSE", 2)


def test_locus_predicate_nulls_fail():
    ok = dict(readMapped=True, primaryAlignment=True, failedVendorQualityChecks=False, duplicateRead=False)
    assert PR.locus_predicate(ok)
    for k in ok:
        assert not PR.locus_predicate(dict(ok, **{k: not ok[k]}))
        assert not PR.locus_predicate(dict(ok, **{k: None}))
        assert not PR.locus_predicate({a: b for a, b in ok.items() if a != k})


@pytest.mark.parametrize("name,rows", [("artificial.sam", 650), ("artificial.realigned.sam", 510),
                                       ("small_realignment_targets.sam", 707), ("reads12.sam", 0),
                                       ("small.sam", 0), ("unmapped.sam", 0)])
def test_golden_sams(name, rows):
    with open(os.path.join(RES, name), "rb") as fh:
        recs = _adam_ref.convert_sam(fh.read())
    out = PR.reads_to_pileups(recs)  # no throw
    assert len(out) == rows
    if rows == 0:
        assert all(r["mismatchingPositions"] is None for r in recs)
    assert all(list(r) == PR.FIELDS for r in out)
