"""The plain-Python restatement of RealignmentTargetFinder
(tests/_realign_targets_ref.py) pinned to the reference's own suite,
IndelRealignmentTargetSuite: its make_read cases, its IndelRange / merge /
overlap unit cases, artificial.sam read by read and all at once, the mason SNP
and indel assertions, and the command's text for one golden."""
import functools
import os

import pytest

import _adam_ref
import _pileup_gen as G
import _pileup_ref as PR
import _realign_targets_gen as RG
import _realign_targets_ref as R
from _realign_targets_ref import IndelRange, Range, SNPRange, Target, make_read

RES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_resources")


@functools.lru_cache(maxsize=None)
def golden_records(name):
    with open(os.path.join(RES, name), "rb") as fh:
        return _adam_ref.convert_sam(fh.read(), G.run_date)


# ---- "checking simple ranges", "checking simple realignment target", "joining simple realignment targets" ----

def test_simple_ranges():
    range1 = IndelRange(Range(1, 4), Range(1, 10))
    range2 = IndelRange(Range(1, 4), Range(40, 50))
    range3 = SNPRange(5, Range(40, 50))
    assert range1 != range2
    assert range1.compare_range(range2) == 0
    assert range1.compare(range2) == -1
    assert range1.compare_read_range(range2) == -1
    assert range2.compare_read_range(range3) == 0
    assert range1.merge(range2).readRange == Range(1, 50)


def test_simple_realignment_target():
    range1 = IndelRange(Range(1, 4), Range(1, 10))
    range2 = IndelRange(Range(1, 4), Range(40, 50))
    range3 = IndelRange(Range(6, 14), Range(80, 90))
    range4 = IndelRange(Range(2, 4), Range(60, 70))
    target1 = Target({range1, range2}, set())
    target2 = Target({range3, range4}, set())
    assert target1.readRange == Range(1, 50)
    assert R.overlap(target1, target1) is True
    assert R.overlap(target1, target2) is False
    assert target2.readRange == Range(60, 90)


def test_joining_simple_realignment_targets():
    target1 = Target({IndelRange(Range(10, 15), Range(1, 20))}, set())
    target2 = Target({IndelRange(Range(10, 15), Range(6, 25))}, set())
    merged = target1.merge(target2)
    assert merged.readRange == Range(1, 25)
    assert merged.indels() == [IndelRange(Range(10, 15), Range(1, 25))]


def test_overlap_is_the_four_clauses():
    def t(a, b):
        return Target({IndelRange(Range(a, a), Range(a, b))}, set())
    assert R.overlap(t(1, 20), t(1, 5))        # the same start
    assert R.overlap(t(1, 20), t(20, 30))      # a.end == b.start
    assert R.overlap(t(1, 20), t(10, 15))      # b inside a
    assert not R.overlap(t(1, 20), t(10, 30))  # a partial overlap is none
    assert not R.overlap(t(1, 20), t(21, 30))


# ---- the make_read cases ----

def test_read_with_deletion():
    (t,) = R.find_targets([make_read(3, "2M3D2M", "2^AAA2", 4)])
    assert t.indels() == [IndelRange(Range(5, 7), Range(3, 9))] and not t.snpSet


def test_read_with_insertion():
    (t,) = R.find_targets([make_read(3, "2M3I2M", "4", 7)])
    assert t.indels() == [IndelRange(Range(5, 5), Range(3, 6))] and not t.snpSet


def test_three_intersecting_reads_same_indel():
    (t,) = R.find_targets([make_read(1, "4M3D2M", "4^AAA2", 6), make_read(2, "3M3D2M", "3^AAA2", 5),
                           make_read(3, "2M3D2M", "2^AAA2", 4)])
    assert t.indels() == [IndelRange(Range(5, 7), Range(1, 9))]


def test_three_intersecting_reads_two_different_indels():
    (t,) = R.find_targets([make_read(1, "2M2D4M", "2^AA4", 6, 0), make_read(1, "2M2D2M2D2M", "2^AA2^AA2", 6, 1),
                           make_read(5, "2M2D4M", "2^AA4", 6, 2)])
    assert t.indels() == [IndelRange(Range(3, 4), Range(1, 10)), IndelRange(Range(7, 8), Range(1, 12))]
    assert t.readRange == Range(1, 12)


def test_two_disjoint_reads():
    a, b = R.find_targets([make_read(1, "2M2D2M", "2^AA2", 4), make_read(7, "2M2D2M", "2^AA2", 4)])
    assert a.indels() == [IndelRange(Range(3, 4), Range(1, 6))]
    assert b.indels() == [IndelRange(Range(9, 10), Range(7, 12))]


def test_fold_depends_on_tie_order_and_the_declared_order_decides():
    # a running target [1,20], then candidates [10,15] and [10,30] with the same start
    def cand(a, b, position):
        return Target({IndelRange(Range(position, position), Range(a, b))}, set(), position)
    first, inside, beyond = cand(1, 20, 5), cand(10, 15, 12), cand(10, 30, 14)
    one = R.join_targets(R.join_targets([first], [inside]), [beyond])
    other = R.join_targets(R.join_targets([first], [beyond]), [inside])
    assert [t.readRange for t in one] == [Range(1, 20), Range(10, 30)]
    assert [t.readRange for t in other] == [Range(1, 20), Range(10, 30)]
    assert len(one[0].indelSet) == 2 and len(other[0].indelSet) == 1  # [10,15] merged left, or into [10,30]


# ---- the goldens ----

def test_mason_rods_matches_mismatches_indels():
    rods = R.group_rods(PR.reads_to_pileups(golden_records("small_realignment_targets.sam")))
    x = [(R.extract_indels(r), R.extract_matches(r), R.extract_mismatches(r)) for r in rods]
    # the first read has CIGAR 100M and MD 92T7
    assert all(len(i) == 0 for i, _, _ in x[0:100])
    assert all(len(m) == 1 and len(mm) == 0 for _, m, mm in x[0:92])
    assert (len(x[92][1]), len(x[92][2])) == (0, 1)
    assert all(len(m) == 1 and len(mm) == 0 for _, m, mm in x[93:100])
    # the second read has CIGAR 32M1D33M1I34M and MD 0G24A6^T67
    assert all(len(i) == 0 for i, _, _ in x[100:132])
    assert (len(x[100][1]), len(x[100][2])) == (0, 1)
    assert all(len(m) == 1 and len(mm) == 0 for _, m, mm in x[101:125])
    assert (len(x[125][1]), len(x[125][2])) == (0, 1)
    assert all(len(m) == 1 and len(mm) == 0 for _, m, mm in x[126:132])
    assert tuple(map(len, x[132])) == (1, 0, 0)
    assert all(tuple(map(len, r)) == (0, 1, 0) for r in x[133:166])
    assert tuple(map(len, x[166])) == (1, 1, 0)


def test_artificial_reads_one_by_one():
    want = {5: (34, 43), 10: (54, 63), 15: (34, 43), 20: (54, 63), 25: (34, 43)}
    for rec in golden_records("artificial.sam"):
        targets = R.find_targets([rec])
        if rec["start"] < 105:
            assert len(targets) == 1
            head = targets[0].indels()[0]
            end = rec["start"] + sum(n for n, op in PR.decode_cigar(rec["cigar"]) if op in "MDN=X")
            assert head.readRange == Range(rec["start"], end - 1)
            assert (head.indelRange.start, head.indelRange.end) == want[rec["start"]]


@pytest.mark.parametrize("name,reads,rows,rods,targets", [("artificial.sam", 10, 650, 30, 1),
                                                          ("small_realignment_targets.sam", 7, 707, 17, 7),
                                                          ("artificial.realigned.sam", 10, 510, 20, 1),
                                                          ("reads12.sam", 200, 0, 0, 0), ("small.sam", 20, 0, 0, 0),
                                                          ("unmapped.sam", 200, 0, 0, 0)])
def test_golden_counts(name, reads, rows, rods, targets):
    recs = golden_records(name)
    got_rows = PR.reads_to_pileups(recs)
    cands = [t for t in map(R.target_of_rod, R.group_rods(got_rows)) if not t.is_empty()]
    assert (len(recs), len(got_rows), len(cands), len(R.find_targets(recs))) == (reads, rows, rods, targets)


def test_artificial_reads_all_at_once():
    targets = R.find_targets(golden_records("artificial.sam"))
    only_indels = [t for t in targets if t.indelSet]
    assert len(only_indels) == 1
    (t,) = only_indels
    assert t.readRange == Range(5, 94)
    assert [i.indelRange for i in t.indels()] == [Range(34, 43), Range(54, 63)]


def test_mason_snp_targets():
    targets = R.find_targets(golden_records("small_realignment_targets.sam"))
    only_snps = [t for t in targets if t.snpSet]
    assert [s.snpSite for s in only_snps[0].snps()] == [701384]
    assert [s.snpSite for s in only_snps[1].snps()] == [702257, 702282]
    assert [s.snpSite for s in only_snps[2].snps()] == [807733]
    assert [s.snpSite for s in only_snps[4].snps()] == [869572, 869673]


def test_mason_indel_targets():
    targets = R.find_targets(golden_records("small_realignment_targets.sam"))
    only_indels = [t for t in targets if t.indelSet]
    assert [i.indelRange for i in only_indels[0].indels()] == [Range(702289, 702289), Range(702323, 702323)]
    assert [i.indelRange for i in only_indels[1].indels()] == [Range(807755, 807755)]
    assert [i.indelRange for i in only_indels[5].indels()] == [Range(869644, 869647)]
    assert [t.indels()[0].indelRange.start for t in only_indels] == [702289, 807755, 808684, 857250, 858175, 869644]


def test_command_text_of_a_golden():
    targets = R.find_targets(golden_records("small_realignment_targets.sam"))
    assert R.text(targets) == ("T 701292 701391 0 1\nS 701384 701292 701391\n"
                               "T 702257 702356 2 2\nI 702289 702289 702257 702356\nI 702323 702323 702257 702356\n"
                               "S 702257 702257 702356\nS 702282 702257 702356\n"
                               "T 807721 807821 1 1\nI 807755 807755 807721 807821\nS 807733 807721 807821\n"
                               "T 808593 808693 1 0\nI 808684 808684 808593 808693\n"
                               "T 857175 857273 1 1\nI 857250 857250 857175 857273\nS 857248 857175 857273\n"
                               "T 858097 858195 1 0\nI 858175 858175 858097 858195\n"
                               "T 869571 869674 1 2\nI 869644 869647 869571 869674\nS 869572 869571 869674\n"
                               "S 869673 869571 869674\n")
    assert R.text(targets, targets_only=True).count("\n") == 7
    # the module's formatter prints the same from the arrays
    from adam_amd.realignment_targets import format_targets
    assert format_targets(R.as_arrays(targets)) == R.text(targets)
    assert format_targets(R.as_arrays(targets), targets_only=True) == R.text(targets, targets_only=True)
    assert format_targets(R.as_arrays([])) == ""


def test_single_rod_keeps_two_ranges_a_merged_target_one():
    ins = [RG.read(100, "6M1I6M", "12"), RG.read(102, "4M1I6M", "10")]
    (t,) = R.find_targets(RG.records(RG.sam_text(ins)))
    assert t.indels() == [IndelRange(Range(106, 106), Range(100, 111)), IndelRange(Range(106, 106), Range(102, 111))]
    dele = [RG.read(100, "6M2D6M", "6^AA6"), RG.read(102, "4M2D6M", "4^AA6")]
    (t,) = R.find_targets(RG.records(RG.sam_text(dele)))
    assert t.indels() == [IndelRange(Range(106, 107), Range(100, 113))]


def test_int_sums_wrap():
    rod = [dict(rangeOffset=None, numSoftClipped=0, readBase="A", referenceBase="A", sangerQuality=2 ** 30,
                position=7, readStart=1, readEnd=9) for _ in range(2)]
    rod.append(dict(rod[0], referenceBase="C", sangerQuality=1))
    # matchQuality wraps to -2^31: the ratio is negative, below the threshold
    assert R.target_of_rod(rod).is_empty()
