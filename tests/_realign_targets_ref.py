"""RealignmentTargetFinder restated in plain Python: the yardstick of the
realignment-target tests.

RealignmentTargetFinder.findTargets / joinTargets (adam-core/.../algorithms/
realignmenttarget/RealignmentTargetFinder.scala:54-101) over
IndelRealignmentTarget (IndelRealignmentTarget.scala:41-101 TargetOrdering,
126-165 IndelRange, 194-231 SNPRange, 251-437 the target, its apply, merge and
RangeAccumulator), written from the Scala, statement by statement, over the
ADAMPileup rows ``_pileup_ref.reads_to_pileups`` returns.  Nothing here knows
how the device does it.

Where the reference leaves an order to Spark or to a hash set, this project
declares one (include/adam_sam.h):

* candidates are folded ascending by ``(readRange.start, position)``;
* a target's indel ranges ascend by ``(indelStart, indelEnd, readStart,
  readEnd)``, its SNP ranges by ``(site, readStart, readEnd)``;
* targets ascend by start, which the fold gives.
"""
from __future__ import annotations

from typing import Dict, FrozenSet, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

import _pileup_ref as PR

MISMATCH_THRESHOLD = 0.15


class Range(NamedTuple):
    """NumericRange.Inclusive[Long](start, end, 1)"""
    start: int
    end: int


class IndelRange(NamedTuple):
    indelRange: Range
    readRange: Range

    def compare_range(self, other) -> int:
        if self.indelRange.start != other.indelRange.start:
            return _cmp(self.indelRange.start, other.indelRange.start)
        return _cmp(self.indelRange.end, other.indelRange.end)

    def compare_read_range(self, other) -> int:
        if self.readRange.start != other.readRange.start:
            return _cmp(self.readRange.start, other.readRange.start)
        return _cmp(self.readRange.end, other.readRange.end)

    def compare(self, other) -> int:
        c = self.compare_range(other)
        return c if c != 0 else self.compare_read_range(other)

    def merge(self, ir: "IndelRange") -> "IndelRange":
        assert self.indelRange == ir.indelRange
        return IndelRange(self.indelRange, Range(min(self.readRange.start, ir.readRange.start),
                                                 max(self.readRange.end, ir.readRange.end)))


class SNPRange(NamedTuple):
    snpSite: int
    readRange: Range

    def compare_range(self, other) -> int:
        return _cmp(self.snpSite, other.snpSite)

    def compare_read_range(self, other) -> int:
        if self.readRange.start != other.readRange.start:
            return _cmp(self.readRange.start, other.readRange.start)
        return _cmp(self.readRange.end, other.readRange.end)

    def compare(self, other) -> int:
        c = self.compare_range(other)
        return c if c != 0 else self.compare_read_range(other)


def _cmp(a: int, b: int) -> int:
    return -1 if a < b else (1 if a > b else 0)


def _int32(v: int) -> int:
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


def extract_indels(rod: Sequence[dict]) -> List[dict]:
    return [r for r in rod if r["rangeOffset"] is not None]


def extract_matches(rod: Sequence[dict]) -> List[dict]:
    return [r for r in rod if r["rangeOffset"] is None and r["numSoftClipped"] == 0
            and r["readBase"] == r["referenceBase"]]


def extract_mismatches(rod: Sequence[dict]) -> List[dict]:
    return [r for r in rod if r["rangeOffset"] is None and r["numSoftClipped"] == 0
            and r["readBase"] != r["referenceBase"]]


class Target:
    """IndelRealignmentTarget(indelSet, snpSet); `position` is the rod's (of a
    merged target: its first candidate's), kept for the declared fold order.
    `n_rods` and `collapsed` are bookkeeping for the tests only: how many
    candidates the target was folded from, and whether a merge ever replaced
    ranges of equal indelRange by their hull."""

    def __init__(self, indel_set: FrozenSet[IndelRange], snp_set: FrozenSet[SNPRange], position: int = -1,
                 n_rods: int = 1, collapsed: bool = False):
        self.indelSet = frozenset(indel_set)
        self.snpSet = frozenset(snp_set)
        self.position = position
        self.n_rods = n_rods
        self.collapsed = collapsed

    @property
    def readRange(self) -> Range:
        rs = [i.readRange for i in self.indelSet] + [s.readRange for s in self.snpSet]
        a = rs[0]
        for b in rs[1:]:
            a = Range(min(a.start, b.start), max(a.end, b.end))
        return a

    def is_empty(self) -> bool:
        return not self.indelSet and not self.snpSet

    def merge(self, target: "Target") -> "Target":
        current = sorted(self.indelSet | target.indelSet,
                         key=lambda i: (i.indelRange.start, i.indelRange.end, i.readRange.start, i.readRange.end))
        # RangeAccumulator
        data: List[IndelRange] = []
        previous: Optional[IndelRange] = None
        for cur in current:
            if previous is None:
                previous = cur
            elif previous.compare_range(cur) == 0:
                previous = previous.merge(cur)
            else:
                data.insert(0, previous)
                previous = cur
        merged = frozenset(data) if previous is None else frozenset(data) | {previous}
        return Target(merged, self.snpSet | target.snpSet, self.position, self.n_rods + target.n_rods,
                      self.collapsed or target.collapsed or len(merged) < len(current))

    # the declared element orders
    def indels(self) -> List[IndelRange]:
        return sorted(self.indelSet, key=lambda i: (i.indelRange.start, i.indelRange.end, i.readRange.start,
                                                    i.readRange.end))

    def snps(self) -> List[SNPRange]:
        return sorted(self.snpSet, key=lambda s: (s.snpSite, s.readRange.start, s.readRange.end))


def overlap(a: Target, b: Target) -> bool:
    """TargetOrdering.overlap, the four clauses as written"""
    ar, br = a.readRange, b.readRange
    return ((ar.start >= br.start and ar.start <= br.end) or
            (ar.end >= br.start and ar.end <= br.start) or
            (ar.start >= br.start and ar.end <= br.end) or
            (br.start >= ar.start and br.end <= ar.end))


def target_of_rod(rod: Sequence[dict]) -> Target:
    """IndelRealignmentTarget.apply(rod)"""

    def read_range(p):
        return Range(int(p["readStart"]), int(p["readEnd"]) - 1)

    def map_event(p) -> IndelRange:
        if p["readBase"] is None:  # deletion
            return IndelRange(Range(p["position"] - p["rangeOffset"],
                                    p["position"] + p["rangeLength"] - p["rangeOffset"] - 1), read_range(p))
        return IndelRange(Range(p["position"], p["position"]), read_range(p))

    def map_point(p) -> SNPRange:
        return SNPRange(p["position"], read_range(p))

    indels = extract_indels(rod)
    matches = extract_matches(rod)
    mismatches = extract_mismatches(rod)
    match_quality = 0
    for m in matches:
        match_quality = _int32(match_quality + m["sangerQuality"])
    mismatch_quality = 0
    for m in mismatches:
        mismatch_quality = _int32(mismatch_quality + m["sangerQuality"])
    position = rod[0]["position"]
    if match_quality == 0 or float(mismatch_quality) / float(match_quality) >= MISMATCH_THRESHOLD:
        return Target(frozenset(map(map_event, indels)), frozenset(map(map_point, mismatches)), position)
    return Target(frozenset(map(map_event, indels)), frozenset(), position)


def join_targets(first: List[Target], second: List[Target]) -> List[Target]:
    """joinTargets over two sets sorted by start (lists here: a TreeSet under
    TargetOrdering holds one target per start, and the fold never offers a
    second one with a start already present without merging it)"""
    while True:
        if first and not second:
            return first
        if not first and second:
            return second
        if not overlap(first[-1], second[0]):
            return first + second
        first = first[:-1] + [first[-1].merge(second[0])]
        second = second[1:]


def group_rods(rows: Sequence[dict]) -> List[List[dict]]:
    """groupBy(_.getPosition): referenceId is not part of the key"""
    rods: Dict[int, List[dict]] = {}
    for r in rows:
        rods.setdefault(r["position"], []).append(r)
    return [rods[p] for p in sorted(rods)]


def find_targets_of_rows(rows: Sequence[dict]) -> List[Target]:
    cands = [t for t in map(target_of_rod, group_rods(rows)) if not t.is_empty()]
    cands.sort(key=lambda t: (t.readRange.start, t.position))
    out: List[Target] = []
    for t in cands:
        out = join_targets(out, [t]) if out else [t]
    return out


def find_targets(recs: Sequence[dict]) -> List[Target]:
    """RealignmentTargetFinder(reads); PileupThrow as reads2ref, and
    UNSUPPORTED for a read with rows and a start below 0 (the device path's
    limit, declared)"""
    rows: List[dict] = []
    for i, rec in enumerate(recs):
        try:
            got = PR.read_to_pileups(rec)
        except PR.PileupThrow as e:
            raise PR.PileupThrow(e.status, str(e), i) from None
        if got and rec["start"] < 0:
            raise PR.PileupThrow("UNSUPPORTED", "start below 0", i)
        rows.extend(got)
    return find_targets_of_rows(rows)


COLUMNS = ("target_start", "target_end", "indel_offset", "snp_offset", "indel_start", "indel_end", "indel_read_start",
           "indel_read_end", "snp_site", "snp_read_start", "snp_read_end")


def as_arrays(targets: Sequence[Target]) -> Dict[str, np.ndarray]:
    """the targets in the layout ``adam_amd.realignment_targets`` returns"""
    c: Dict[str, list] = {k: [] for k in COLUMNS}
    c["indel_offset"].append(0)
    c["snp_offset"].append(0)
    for t in targets:
        rr = t.readRange
        c["target_start"].append(rr.start)
        c["target_end"].append(rr.end)
        for i in t.indels():
            c["indel_start"].append(i.indelRange.start)
            c["indel_end"].append(i.indelRange.end)
            c["indel_read_start"].append(i.readRange.start)
            c["indel_read_end"].append(i.readRange.end)
        for s in t.snps():
            c["snp_site"].append(s.snpSite)
            c["snp_read_start"].append(s.readRange.start)
            c["snp_read_end"].append(s.readRange.end)
        c["indel_offset"].append(len(c["indel_start"]))
        c["snp_offset"].append(len(c["snp_site"]))
    return {k: np.asarray(v, np.int64) for k, v in c.items()}


def text(targets: Sequence[Target], targets_only: bool = False) -> str:
    """the CLI's text"""
    out = []
    for t in targets:
        rr = t.readRange
        out.append("T %d %d %d %d\n" % (rr.start, rr.end, len(t.indelSet), len(t.snpSet)))
        if targets_only:
            continue
        for i in t.indels():
            out.append("I %d %d %d %d\n" % (i.indelRange.start, i.indelRange.end, i.readRange.start, i.readRange.end))
        for s in t.snps():
            out.append("S %d %d %d\n" % (s.snpSite, s.readRange.start, s.readRange.end))
    return "".join(out)


def make_read(start: int, cigar: str, md: str, length: int, id: int = 0, seq: Optional[str] = None,
              qual: Optional[str] = None) -> dict:
    """IndelRealignmentTargetSuite.make_read"""
    s = "A" * length if seq is None else seq
    return dict(readName="read%d" % id, start=start, readMapped=True, cigar=cigar, sequence=s,
                readNegativeStrand=False, mapq=60, qual=s if qual is None else qual, mismatchingPositions=md)
