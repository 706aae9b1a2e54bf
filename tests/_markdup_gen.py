"""One source of reads for every MarkDuplicates entry point.  TEST INFRASTRUCTURE.

Reads are oracle/markdup.py's dicts (name, library, rg, mapped, primary,
paired, mate_mapped, neg, ref, start, qual, cigar).  The same reads are
rendered as SAM text (`sam_text`), as BAM (`bam_bytes`) and as the pyarrow
table `ArrowReads(..., markdup=True)` loads (`arrow_table`); `host_mark` runs
the library's host form bqsr_mark_duplicates over them.

`CASES` holds the hand-built cases (the reference's MarkDuplicatesSuite among
them: `REFERENCE_SUITE`, which tests/test_markdup.py runs one by one),
`concat` lays cases side by side so that they cannot meet, and `random_reads`
draws a dense random set from the same features.

A read is SAM-expressible (`sam_ok`) when SAM text can hold it: a printable
QNAME, a non-empty QUAL, the library its read group's @RG line names, and a
position when it is mapped.  Everything else is for the Arrow rendering only.
"""
import os
import tempfile

import numpy as np

import markdup as M  # oracle/markdup.py (tests/conftest.py puts oracle/ on sys.path)
from adam_amd import records as R

OPS = "MIDNSHP=X"
CONTIGS = ["ctg%02d" % i for i in range(12)]  # ref = the @SQ index
# read groups by id (ids follow the sorted ID strings, SAMRecordConverter's RecordGroupDictionary):
# two share an LB, one has none, and the library ranks (sorted LB: libM < library bar) run against the ids
RG_IDS = ["rgA", "rgB", "rgC", "rgD"]
RG_LIB = {0: "library bar", 1: None, 2: "libM", 3: "library bar"}
RG_HEADER_ORDER = [2, 0, 3, 1]  # the @RG lines' order in the text: neither id nor library order
CASE_SPAN = 2000  # concat: case i's positions are shifted by i * CASE_SPAN


def header(contigs=CONTIGS, rg_ids=RG_IDS, rg_lib=RG_LIB, rg_order=RG_HEADER_ORDER):
    """The header text: an @SQ line per contig, an @RG line per read group
    (rg_ids[g]: the ID of read group id g, sorted; rg_lib[g]: its LB or None),
    written in rg_order."""
    assert list(rg_ids) == sorted(rg_ids)
    lines = ["@HD\tVN:1.4"] + ["@SQ\tSN:%s\tLN:100000000" % c for c in contigs]
    for g in rg_order:
        lines.append("@RG\tID:%s%s" % (rg_ids[g], "" if rg_lib[g] is None else "\tLB:" + rg_lib[g]))
    return ("\n".join(lines) + "\n").encode("latin-1")


def parse_cigar(text):
    return [(int(e) >> 4, OPS[int(e) & 15]) for e in R.parse_cigar(text)]


def query_len(cigar):
    return sum(n for n, op in cigar if op in "MIS=X")


def ref_len(cigar):
    return sum(n for n, op in cigar if op in M.CONSUMES_REF)


_DEFAULT = object()


def rd(name, ref, pos, cigar="100M", neg=False, rg=0, phred=20, qual=None, primary=True, mapped=True, paired=False,
       mate_mapped=False, library=_DEFAULT):
    """A read whose 5' position (MarkDuplicates' key) is `pos`: the start is
    worked back from it through the clips (forward) or the reference span and
    the trailing clips (reverse).  pos None: no position (ref and start null)."""
    cig = parse_cigar(cigar) if isinstance(cigar, str) else list(cigar)
    if pos is None:
        start = None
    elif not neg:
        lead = 0
        for n, op in cig:
            if op not in M.CLIPPED:
                break
            lead += n
        start = pos + lead
    else:
        trail = 0
        for n, op in reversed(cig):
            if op not in M.CLIPPED:
                break
            trail += n
        start = pos - ref_len(cig) - trail
    n = query_len(cig) if cig else 10
    r = dict(name=name, library=(RG_LIB[rg] if rg is not None else None) if library is _DEFAULT else library, rg=rg,
             mapped=mapped, primary=primary, paired=paired, mate_mapped=mate_mapped and paired, neg=neg, ref=ref,
             start=start, qual=chr(phred + 33) * n if qual is None else qual, cigar=cig)
    if mapped and pos is not None:
        assert start >= 0 and M.five_prime(r) == pos
    return r


def mates(name, a, b, **kw):
    """Two reads under one name, flagged as a pair with mapped mates; a and b
    are rd()'s (ref, pos[, cigar]) with the first forward, the second reverse."""
    out = []
    for k, spec in enumerate((a, b)):
        ref, pos = spec[:2]
        out.append(rd(name, ref, pos, spec[2] if len(spec) > 2 else "100M", neg=k == 1, paired=True,
                      mate_mapped=True, **kw))
    return out


# ---- the reference's MarkDuplicatesSuite (core/.../rdd/MarkDuplicatesSuite.scala:27-166) ----

def mapped(ref, pos, name, phred=20, clipped=0, primary=True, neg=False):
    """MarkDuplicatesSuite.createMappedRead (:27-48)."""
    cigar = [(clipped, "S"), (100 - clipped, "M")] if clipped else [(100, "M")]
    return dict(name=name, library="library bar", rg=0, mapped=True, primary=primary, paired=False,
                mate_mapped=False, neg=neg, ref=ref, start=pos, qual=chr(phred + 33) * 100, cigar=cigar)


def unmapped():
    """createUnmappedRead (:23-25): only readMapped = false is set."""
    return dict(name=None, library=None, rg=None, mapped=False, primary=False, paired=False, mate_mapped=False,
                neg=False, ref=0, start=0, qual="", cigar=[])


def pair(ref1, pos1, ref2, pos2, name, phred=20):
    """createPair (:50-72)."""
    a = mapped(ref1, pos1, name=name, phred=phred)
    b = mapped(ref2, pos2, name=name, phred=phred, neg=True)
    for r in (a, b):
        r["paired"] = True
        r["mate_mapped"] = True
    return [a, b]


def _read_pairs():
    reads = pair(0, 10, 0, 210, name="best", phred=30)
    for i in range(10):
        reads += pair(0, 10, 0, 210, name="poor%d" % i)
    return reads


# name -> (reads, the suite's own expectation per read)
REFERENCE_SUITE = {
    "single_read": lambda: ([mapped(0, 100, "only")], [False]),
    "reads_at_different_positions": lambda: ([mapped(0, 42, "a"), mapped(0, 43, "b")], [False, False]),
    "reads_at_the_same_position": lambda: (
        [mapped(1, 42, phred=30, name="best")] + [mapped(1, 42, name="poor%d" % i) for i in range(10)],
        [False] + [True] * 10),
    "reads_at_the_same_position_with_clipping": lambda: (
        [mapped(1, 42, phred=30, name="best")] +
        [mapped(1, 44, clipped=2, name="poorClipped%d" % i) for i in range(5)] +
        [mapped(1, 42, name="poorUnclipped%d" % i) for i in range(5)],
        [False] + [True] * 10),
    "reads_on_reverse_strand": lambda: (
        [mapped(10, 42, neg=True, phred=30, name="best")] +
        [mapped(10, 42, neg=True, name="poor%d" % i) for i in range(7)],
        [False] + [True] * 7),
    "unmapped_reads": lambda: ([unmapped() for _ in range(10)], [False] * 10),
    "read_pairs": lambda: (_read_pairs(), [False, False] + [True] * 20),
    "read_pairs_with_fragments": lambda: (
        [mapped(2, 33, phred=40, name="fragment%d" % i) for i in range(10)] + pair(2, 33, 2, 200, name="pair"),
        [True] * 10 + [False, False]),
}


# ---- hand-built cases: name -> (reads, expectation per read) ----
# The expectation is written down from the rules, not taken from any code;
# the tests hold the oracle to it as well as the library.

def _five_prime_forward():
    reads = [rd("a", 0, 100, "100M", phred=30), rd("b", 0, 100, "5S95M"), rd("c", 0, 100, "2H3S95M"),
             rd("d", 0, 101, "100M"), rd("e", 0, 102, "3S95M")]  # e: where c lands if H were no clip
    assert [r["start"] for r in reads[:3]] == [100, 105, 105]
    return reads, [False, True, True, False, False]


def _five_prime_reverse():
    cigars = ["100M", "95M5S", "95M3S2H", "40M5D55M", "40M5N55M", "40=5X50M5I", "50M2P50M", "40M10I50M"]
    reads = [rd("r%d" % i, 0, 700, c, neg=True, phred=30 if i == 0 else 20) for i, c in enumerate(cigars)]
    # decoys where a wrong end would land: N, D not counted (695), clips not counted (695, 698), I or P counted
    reads += [rd("x%d" % i, 0, p, "100M", neg=True, phred=10) for i, p in enumerate((695, 698, 702, 705, 710))]
    return reads, [False] + [True] * 7 + [False] * 5


def _forward_and_reverse_same_position():
    reads = [rd("f", 0, 300), rd("r", 0, 300, neg=True), rd("f2", 0, 300, phred=10)]
    return reads, [False, False, True]


def _negative_unclipped_start():
    reads = [rd("a", 0, -7, "7S93M", phred=30), rd("b", 0, -7, "7S93M"), rd("c", 0, 0, "100M"),
             rd("d", 0, -3, "3S97M"), rd("e", 0, -7, "2H5S95M", phred=10)]
    assert all(r["start"] == 0 for r in reads)
    return reads, [False, True, False, False, True]


def _same_position_two_contigs():
    reads = [rd("a", 0, 500), rd("b", 1, 500), rd("c", 1, 500, phred=10), rd("d", 2, 500, neg=True),
             rd("e", 1, 500, neg=True)]
    return reads, [False, False, True, False, False]


def _cross_contig_pairs():
    # every pair: the higher-contig mate first in the input, so left and right swap
    def cross(name, hi, lo, phred):
        b, a = mates(name, lo, hi, phred=phred)  # a: reverse read on the higher contig
        return [a, b]
    reads = (cross("p1", (1, 700), (0, 200), 30) + cross("p3", (2, 700), (0, 200), 30) +
             cross("p2", (1, 700), (0, 200), 20) + cross("p4", (2, 700), (0, 200), 20) +  # runs interleaved in the input
             cross("p5", (1, 700), (0, 300), 10) +  # the same higher mate, another lower mate: no duplicate
             cross("p6", (2, 700), (1, 200), 10))   # the same right mate and left position on another contig
    return reads, [False] * 4 + [True] * 4 + [False] * 4


def _buckets_of_three_and_four():
    t = [rd("t", 0, 100, phred=20), rd("t", 0, 400, neg=True, phred=20), rd("t", 0, 900, phred=40)]  # 8000
    u = mates("u", (0, 100), (0, 400), phred=30)  # 6000: above t's first two, below all three
    v = [rd("v", 1, 100, phred=15), rd("v", 1, 400, neg=True, phred=15), rd("v", 0, 5, phred=15),
         rd("v", 2, 500, neg=True, phred=15)]  # 6000
    w = mates("w", (1, 100), (1, 400), phred=25)  # 5000
    x = mates("x", (1, 100), (1, 400), phred=35)  # 7000
    return t + u + v + w + x, [False] * 3 + [True] * 2 + [True] * 4 + [True] * 2 + [False] * 2


def _buckets_without_primary_reads():
    reads = [rd("s", 0, 100, primary=False), rd("s", 0, 100, primary=False, phred=40),  # secondary only
             rd("n", None, None, "", mapped=False), rd("n", None, None, "", mapped=False),  # unmapped only
             rd("z", None, None, "", mapped=False, primary=False),  # FLAG 0 in SAM text: nothing is set
             rd("x", 0, 100, phred=30), rd("y", 0, 100)]
    return reads, [False] * 5 + [False, True]


def _unmapped_mate_first():
    reads = [rd("m", None, None, "", mapped=False, paired=True, mate_mapped=True),
             rd("m", 0, 100, paired=True, mate_mapped=False),
             rd("k", 0, 100, phred=30),
             rd("j", 0, 200, paired=True, mate_mapped=False, phred=30),  # the mapped read first
             rd("j", 0, 200, "", mapped=False, paired=True, mate_mapped=True),  # unmapped, placed at its mate
             rd("i", 0, 200)]
    return reads, [False, True, False, False, False, True]


def _secondary_before_primary():
    reads = [rd("k", 0, 150, primary=False, phred=40), rd("j", 0, 100, phred=30), rd("k", 0, 100),
             rd("j", 0, 170, primary=False),  # the winner's secondary read is a duplicate as well
             rd("h", 0, 300, primary=False), rd("h", 0, 300, phred=10)]  # alone at its position: only the secondary
    return reads, [True, False, True, True, True, False]


def _one_name_in_several_read_groups():
    reads = [rd("z", 0, 100, rg=0, phred=30), rd("z", 0, 100, rg=3), rd("z", 0, 100, rg=None, phred=30),
             rd("y", 0, 100, rg=None), rd("z", 0, 100, rg=2), rd("z", 0, 100, rg=2, phred=40)]  # rg 2: one bucket
    return reads, [False, True, False, True, False, False]


def _names_that_are_prefixes():
    reads = [rd("q1", 0, 100, phred=30), rd("q10", 0, 100), rd("q", 0, 100, phred=10), rd("q100", 0, 100, phred=10)]
    return reads, [False, True, True, True]


def _names_that_are_prefixes_control_char():
    reads = [rd("w1", 0, 100, phred=30), rd("w1\x01", 0, 100), rd("w1\x01\x01", 0, 100, phred=10)]
    return reads, [False, True, True]


LONG_NAME = "L" + "".join(chr(33 + (7 * i) % 31) for i in range(252))  # 253 chars of '!'..'?'


def _name_lengths():
    reads = [rd("Z", 0, 100, phred=30), rd(LONG_NAME + "a", 0, 100), rd(LONG_NAME + "b", 0, 100, phred=10),
             rd("Y", 0, 100), rd(LONG_NAME + "a", 0, 500, neg=True)]
    assert len(reads[1]["name"]) == 254
    # the 254-char names differ in their last char alone: "a" is a pair, and every fragment beside a pair is marked
    return reads, [True, False, True, True, False]


def _libraries():
    reads = [rd("a", 0, 100, rg=None, phred=30), rd("b", 0, 100, rg=None),  # no read group: library null
             rd("c", 0, 100, rg=1, phred=25),  # a read group without LB: null as well, the same group
             rd("d", 0, 100, rg=0), rd("e", 0, 100, rg=3, phred=30),  # two read groups, one LB
             rd("f", 0, 100, rg=2), rd("g", 0, 100, rg=2, phred=10)]  # another LB
    return reads, [False, True, True, True, False, False, True]


def _group_with_pairs_and_fragments():
    reads = [rd("f1", 0, 100, phred=40), rd("f2", 0, 100, phred=10)]
    reads += mates("a1", (0, 100), (0, 300), phred=30) + mates("b1", (0, 100), (0, 400), phred=20)
    reads += mates("c1", (0, 100), (1, 500), phred=20) + mates("a2", (0, 100), (0, 300), phred=20)
    reads += mates("b2", (0, 100), (0, 400), phred=30) + mates("c2", (0, 100), (1, 500), phred=20)  # c: a tie
    reads += mates("b3", (0, 100), (0, 400), phred=25) + [rd("f3", 0, 100, phred=41)]
    want = [True, True] + [False] * 2 + [True] * 2 + [False] * 2 + [True] * 2 + [False] * 2 + [True] * 2 + \
        [True] * 2 + [True]
    return reads, want


def _ties():
    reads = [rd("a", 0, 100), rd("b", 0, 100), rd("c", 0, 100), rd("low", 0, 100, phred=10)]
    reads += mates("p", (0, 500), (0, 800)) + mates("q", (0, 500), (0, 800)) + mates("r", (0, 500), (0, 800))
    reads += [rd("z1", 1, 100, phred=10), rd("z2", 1, 100, phred=14)]  # both score 0
    return reads, [False, True, True, True] + [False] * 2 + [True] * 4 + [False, True]


def _score_threshold():
    q15 = chr(33 + 15) + chr(33) * 99  # one base of phred 15: score 15
    reads = [rd("star", 0, 100, qual="*"), rd("p14", 0, 100, phred=14), rd("one15", 0, 100, qual=q15),
             rd("p14b", 1, 100, phred=14), rd("all15", 1, 100, phred=15), rd("one15b", 1, 100, qual=q15)]
    return reads, [True, True, False, True, False, True]


def _score_high_bytes():
    # (char - 33).toByte: 0x80 -> 95, 0xA0 -> 127, 0xA1 -> -128, 0xFF -> -34
    reads = [rd("a1", 0, 100, qual="\xa1" * 100), rd("p20", 0, 100),  # signed: 0 < 2000; unsigned: 12800 > 2000
             rd("ff", 0, 400, qual="\xff" * 100), rd("p20b", 0, 400),
             rd("x80", 0, 700, qual="\x80" * 100), rd("xa0", 0, 700, qual="\xa0" * 100),  # 9500 < 12700
             rd("mix", 1, 100, qual="\xa0\xa1" * 50), rd("p60", 1, 100, phred=60)]  # 6350 > 6000
    return reads, [True, False, True, False, True, False, False, True]


def _empty_qual():
    reads = [rd("e", 0, 100, qual=""), rd("f", 0, 100, qual=chr(33 + 15) + chr(33) * 99), rd("g", 0, 100, qual="")]
    return reads, [True, False, True]


def _null_names():
    reads = [rd(None, 0, 100, rg=2, phred=30, paired=True, mate_mapped=True),
             rd("", 0, 100, rg=2, phred=40, paired=True, mate_mapped=True),
             rd(None, 0, 300, rg=2, neg=True, phred=30, paired=True, mate_mapped=True),
             rd("", 0, 300, rg=2, neg=True, phred=40, paired=True, mate_mapped=True),
             rd(None, 0, 100, rg=3, library="libM", phred=50)]  # another read group: its own bucket, a fragment
    return reads, [True, False, True, False, True]


def _null_library():
    reads = [rd("a", 0, 100, rg=0, library=None, phred=30), rd("b", 0, 100, rg=0), rd("c", 0, 100, rg=0, library=None),
             rd("d", 0, 100, rg=0, phred=10)]
    return reads, [False, False, True, True]


def _libraries_within_one_bucket():
    reads = [rd("m", None, None, "", mapped=False, library="libU"), rd("m", 0, 150, primary=False, library="libS"),
             rd("m", 0, 100, library="libP"),
             rd("o", 0, 100, library="libP", phred=30), rd("o2", 0, 100, library="libS"),
             rd("o3", 0, 100, library="libU", phred=10)]
    return reads, [False, True, True, False, False, False]


CASES = {"negative_unclipped_start": _negative_unclipped_start}  # first: concat leaves its positions as they are
CASES.update({("reference_" + k): v for k, v in REFERENCE_SUITE.items()})
CASES.update({
    "five_prime_forward": _five_prime_forward,
    "five_prime_reverse": _five_prime_reverse,
    "forward_and_reverse_same_position": _forward_and_reverse_same_position,
    "same_position_two_contigs": _same_position_two_contigs,
    "cross_contig_pairs": _cross_contig_pairs,
    "buckets_of_three_and_four": _buckets_of_three_and_four,
    "buckets_without_primary_reads": _buckets_without_primary_reads,
    "unmapped_mate_first": _unmapped_mate_first,
    "secondary_before_primary": _secondary_before_primary,
    "one_name_in_several_read_groups": _one_name_in_several_read_groups,
    "names_that_are_prefixes": _names_that_are_prefixes,
    "names_that_are_prefixes_control_char": _names_that_are_prefixes_control_char,
    "name_lengths": _name_lengths,
    "libraries": _libraries,
    "group_with_pairs_and_fragments": _group_with_pairs_and_fragments,
    "ties": _ties,
    "score_threshold": _score_threshold,
    "score_high_bytes": _score_high_bytes,
    "empty_qual": _empty_qual,
    "null_names": _null_names,
    "null_library": _null_library,
    "libraries_within_one_bucket": _libraries_within_one_bucket,
})
RAW_NAMES = {"name_lengths"}  # names kept as they are by concat (their length is the point)


def case(name):
    """(reads, expectation) of a hand-built case."""
    reads, want = CASES[name]()
    assert len(reads) == len(want), name
    return reads, list(want)


def read_sam_ok(r, rg_lib=RG_LIB):
    n = r["name"]
    return (n is not None and 1 <= len(n) <= 254 and all("!" <= c <= "~" and c != "@" for c in n) and
            r["qual"] != "" and r["library"] == (rg_lib[r["rg"]] if r["rg"] is not None else None) and
            (not r["mapped"] or (r["ref"] is not None and r["start"] is not None)) and
            (r["ref"] is None) == (r["start"] is None) and (r["mate_mapped"] <= r["paired"]) and
            (r["qual"] == "*" or len(r["qual"]) == (query_len(r["cigar"]) if r["cigar"] else len(r["qual"]))))


def sam_ok(reads):
    return all(read_sam_ok(r) for r in reads)


def concat(names=None, sam_only=False):
    """The named cases (all by default) side by side: case i's names carry a
    prefix and its positions are shifted by i * CASE_SPAN, so no two cases
    share a bucket or a position.  Returns (reads, expectation)."""
    reads, want = [], []
    for i, name in enumerate(CASES if names is None else names):
        rs, w = case(name)
        if sam_only and not sam_ok(rs):
            continue
        for r in rs:
            r = dict(r)
            if r["name"] and name not in RAW_NAMES:  # a null and an empty name stay what they are
                r["name"] = "%d:%s" % (i, r["name"])
            if r["start"] is not None:
                r["start"] += i * CASE_SPAN
            reads.append(r)
        want += w
    return reads, want


# ---- renderings ----

def sam_flag(r):
    f = 0
    if r["paired"]:
        f |= 0x1 | (0 if r["mate_mapped"] else 0x8)
    if r["neg"]:
        f |= 0x10
    if not r["mapped"]:
        f |= 0x4
    if not r["primary"]:
        f |= 0x100
    if f == 0x104:
        f = 0  # FLAG 0 sets nothing (SAMRecordConverter.scala:72-100): neither mapped nor primary
    elif f == 0:
        f = 0x200  # a plain forward fragment needs one bit set to be mapped at all
    return f


def sam_line(r, contigs=CONTIGS, rg_ids=RG_IDS, rg_lib=RG_LIB):
    assert read_sam_ok(r, rg_lib), r
    n = query_len(r["cigar"]) if r["cigar"] else (10 if r["qual"] == "*" else len(r["qual"]))
    f = [r["name"], str(sam_flag(r)), "*" if r["ref"] is None else contigs[r["ref"]],
         "0" if r["start"] is None else str(r["start"] + 1), "60",
         "".join("%d%s" % e for e in r["cigar"]) or "*", "*", "0", "0", "A" * n, r["qual"]]
    if r["rg"] is not None:
        f.append("RG:Z:" + rg_ids[r["rg"]])
    return "\t".join(f).encode("latin-1")


def sam_body(reads, contigs=CONTIGS, rg_ids=RG_IDS, rg_lib=RG_LIB):
    return [sam_line(r, contigs, rg_ids, rg_lib) for r in reads]


def sam_text(reads, head=None):
    return (header() if head is None else head) + b"".join(l + b"\n" for l in sam_body(reads))


def bam_bytes(reads, head=None):
    from adam_amd.bam_writer import sam_to_bam
    return sam_to_bam(sam_text(reads, head))


def sam_fields(text):
    return [l.split(b"\t") for l in text.split(b"\n") if l and not l.startswith(b"@")]


def dicts_of_sam(text, contigs=CONTIGS, rg_lib=RG_LIB):
    """The reads of a SAM text as records.read_sam_records loads them, as dicts."""
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "x.sam")
        with open(p, "wb") as fh:
            fh.write(text)
        recs = R.read_sam_records(p)
    ref_of = {c: i for i, c in enumerate(contigs)}
    out = []
    for rec, f in zip(recs, sam_fields(text)):
        flag = int(f[1])
        rg = rec.record_group_id
        out.append(dict(name=rec.read_name, library=rg_lib[rg] if rg is not None else None, rg=rg,
                        mapped=rec.read_mapped, primary=rec.primary_alignment, paired=rec.read_paired,
                        mate_mapped=flag != 0 and bool(flag & 1) and not flag & 8, neg=rec.read_negative_strand,
                        ref=None if rec.reference_name is None else ref_of[rec.reference_name], start=rec.start,
                        qual=rec.qual, cigar=parse_cigar(rec.cigar)))
    return out


def arrow_table(reads):
    """The reads as ADAMRecord columns (adam.avdl names), with MarkDuplicates'
    recordGroupLibrary, mateMapped and referenceId."""
    import pyarrow as pa
    col = lambda k: [r[k] for r in reads]
    cig = [("".join("%d%s" % e for e in r["cigar"]) or None) for r in reads]
    cols = {
        "referenceName": pa.array([None if r["ref"] is None else CONTIGS[r["ref"]] for r in reads], pa.string()),
        "referenceId": pa.array(col("ref"), pa.int32()),
        "start": pa.array(col("start"), pa.int64()),
        "readName": pa.array(col("name"), pa.string()),
        "sequence": pa.array(["A" * query_len(r["cigar"]) if r["cigar"] else None for r in reads], pa.string()),
        "cigar": pa.array(cig, pa.string()),
        "qual": pa.array(col("qual"), pa.string()),
        "recordGroupId": pa.array(col("rg"), pa.int32()),
        "recordGroupLibrary": pa.array(col("library"), pa.string()),
        "readPaired": pa.array(col("paired"), pa.bool_()),
        "readMapped": pa.array(col("mapped"), pa.bool_()),
        "mateMapped": pa.array(col("mate_mapped"), pa.bool_()),
        "readNegativeStrand": pa.array(col("neg"), pa.bool_()),
        "secondOfPair": pa.array([False] * len(reads), pa.bool_()),
        "primaryAlignment": pa.array(col("primary"), pa.bool_()),
        "duplicateRead": pa.array([False] * len(reads), pa.bool_()),
        "mismatchingPositions": pa.array([None] * len(reads), pa.string()),
    }
    return pa.table(cols)


def host_mark(reads):
    """bqsr_mark_duplicates (the library's host form, no device) over the reads."""
    from adam_amd.sam import mark_duplicates
    flags, quals, cigs = [], [], []
    for r in reads:
        f = 0
        f |= R.F_MAPPED if r["mapped"] else 0
        f |= R.F_PRIMARY if r["primary"] else 0
        f |= R.F_PAIRED if r["paired"] else 0
        f |= R.F_NEG_STRAND if r["neg"] else 0
        f |= R.F_HAS_RG if r["rg"] is not None else 0
        flags.append(f)
        quals.append(r["qual"].encode("latin-1"))
        cigs.append([(n << 4) | OPS.index(op) for n, op in r["cigar"]])
    qo = np.zeros(len(reads) + 1, np.uint64)
    np.cumsum([len(q) for q in quals], out=qo[1:])
    co = np.zeros(len(reads) + 1, np.uint64)
    np.cumsum([len(c) for c in cigs], out=co[1:])
    return mark_duplicates([r["name"] for r in reads], [r["library"] for r in reads], flags,
                           [r["mate_mapped"] for r in reads], [r["rg"] or 0 for r in reads],
                           [-1 if r["ref"] is None else r["ref"] for r in reads],
                           [0 if r["start"] is None else r["start"] for r in reads], qo,
                           np.frombuffer(b"".join(quals), np.uint8), co,
                           np.asarray([e for c in cigs for e in c], np.uint32))


# ---- random sets ----

RANDOM_CIGARS = ["60M", "5S55M", "2H3S55M", "30M5D30M", "20M10I30M", "25=5X30M", "30M100N30M", "30M2P30M", "55M5S",
                 "55M3S2H", "4H56M", "1S58M1S"]
RANDOM_POSITIONS = [400 + 25 * k for k in range(40)]
RANDOM_SEEDS = (1, 2, 3)  # with 2000 reads each meets RANDOM_FLOOR (tests/test_markdup_cases.py holds them to it)
SMALL_SEED = 1  # the 300-read set of the one-read-per-partition test
RANDOM_FLOOR = dict(duplicate_primaries=20, duplicate_secondaries=5, fragment_dups_in_paired_groups=5, ties=5,
                    cross_contig_pairs=5, multi_right_groups=1)


def random_reads(n_reads, seed):
    """A dense random set, SAM-expressible: 3 contigs, 4 read groups (and
    none), 40 positions; fragments, pairs (a third across contigs, mates in
    either order), buckets of three, secondary and unmapped reads beside them
    or alone, every CIGAR of RANDOM_CIGARS, a few scores so that ties are
    common, QUAL '*' and bytes above 0x7F.  Names recur only inside a bucket,
    except that some names are used in two read groups."""
    rng = np.random.default_rng(seed)
    reads = []

    def pick(seq):
        return seq[int(rng.integers(0, len(seq)))]

    def position():
        k = int(40 * rng.random() ** 2)  # skewed: the first positions are crowded
        return int(rng.integers(0, 3)), RANDOM_POSITIONS[k]

    def quality(cigar):
        n = query_len(parse_cigar(cigar))
        u = rng.random()
        if u < 0.04:
            return "*"
        if u < 0.10:
            return pick(["\x80", "\xa0", "\xa1", "\xff"]) * n
        if u < 0.18:
            return "".join(chr(33 + int(q)) for q in rng.integers(0, 45, size=n))
        return chr(33 + pick([10, 14, 10, 14, 15, 20, 20, 30])) * n

    def primary(name, rg, ref, pos, neg, **kw):
        c = pick(RANDOM_CIGARS)
        return rd(name, ref, pos, c, neg=neg, rg=rg, qual=quality(c), **kw)

    k = 0
    while len(reads) < n_reads:
        k += 1
        rg = pick([None, 0, 0, 1, 2, 3])
        name = "n%d" % (k if rng.random() < 0.9 else max(1, k - int(rng.integers(1, 30))))  # some names recur
        u = rng.random()
        unit = []
        if u < 0.40:  # a fragment
            ref, pos = position()
            unit.append(primary(name, rg, ref, pos, bool(rng.integers(0, 2)), paired=bool(rng.integers(0, 2))))
        elif u < 0.80:  # a pair, a third of them across contigs
            ref, pos = position()
            ref2, pos2 = position()
            if rng.random() < 0.67:
                ref2 = ref
            a = primary(name, rg, ref, pos, bool(rng.integers(0, 4) == 0), paired=True, mate_mapped=True)
            b = primary(name, rg, ref2, pos2, bool(rng.integers(0, 4) != 0), paired=True, mate_mapped=True)
            unit += [a, b] if rng.random() < 0.5 else [b, a]
        elif u < 0.86:  # three primary reads under one name
            for _ in range(3):
                ref, pos = position()
                unit.append(primary(name, rg, ref, pos, bool(rng.integers(0, 2))))
        elif u < 0.93:  # a mapped read whose mate is unmapped, in either order
            ref, pos = position()
            a = primary(name, rg, ref, pos, bool(rng.integers(0, 2)), paired=True, mate_mapped=False)
            b = rd(name, ref, a["start"] if rng.random() < 0.5 else None, "", mapped=False, rg=rg, paired=True,
                   mate_mapped=True, qual="I" * 10)
            if b["start"] is None:
                b["ref"] = None
            unit += [a, b] if rng.random() < 0.5 else [b, a]
        else:  # no primary read at all
            for _ in range(int(rng.integers(1, 3))):
                if rng.random() < 0.5:
                    ref, pos = position()
                    unit.append(primary(name, rg, ref, pos, bool(rng.integers(0, 2)), primary=False))
                else:
                    unit.append(rd(name, None, None, "", mapped=False, primary=bool(rng.integers(0, 2)), rg=rg,
                                   qual="I" * 10))
        if unit[0]["primary"] and unit[0]["mapped"] and rng.random() < 0.15:  # a secondary read beside them
            ref, pos = position()
            s = primary(name, rg, ref, pos, bool(rng.integers(0, 2)), primary=False)
            unit.insert(int(rng.integers(0, len(unit) + 1)), s)
        reads += unit
    return reads[:n_reads]


def coverage(reads):
    """What the oracle's answer on `reads` exercises (RANDOM_FLOOR's keys)."""
    ties, stats = [], {}
    want = M.mark_duplicates(reads, ties, stats)
    out = dict(duplicate_primaries=sum(w and r["primary"] and r["mapped"] for w, r in zip(want, reads)),
               duplicate_secondaries=sum(w and not r["primary"] and r["mapped"] for w, r in zip(want, reads)),
               ties=len(ties))
    for key in ("fragment_dups_in_paired_groups", "cross_contig_pairs", "multi_right_groups"):
        out[key] = stats.get(key, 0)
    return out
