"""`adam compare -baseqs` (§8 f4): per-base quality concordance of two read
sets, e.g. a reference run's recalibrated reads against this build's.

Restates adam-cli/.../cli/CompareAdam.scala:139-172 (printSummary) over
core/rdd/comparisons/ComparisonTraversalEngine.scala (reads in
SingleReadBuckets keyed by readName, the two inputs joined by name),
core/models/ReadBucket.scala:97-110 (a bucket's reads split into unpaired /
first / second of pair, primary / secondary) and
core/metrics/AvailableComparisons.scala:149-177 (BaseQualityScores: for each
of five categories holding exactly one read on both sides, the pairs
(q1, q2) of the two reads' qualityScores zipped; the histogram's count and
identity, diff% = 100 (count - identity) / count).  qualityScores are
(char - 33).toByte values (RichADAMRecord.scala:43).

Inputs are SAM files read with SAMRecordConverter's flag semantics (flags
only when the FLAG word is non-zero); ``encoding`` is how QUAL bytes map to
Java chars: latin-1 for plain SAM, utf-8 for this build's transform output
(which writes chars above 0x7F as UTF-8).

Below that first part (kept as it was: ``compare_baseqs`` and its helpers)
are all five comparisons of AvailableComparisons.scala:44-177 and the filters
of `findreads` -- ``compare_host`` in Python over SAM text (the path without
a GPU and the tests' oracle) and ``compare_device`` over SAM, BAM or ADAM
Parquet on the device (csrc/compare.hip); ``compare`` picks the device when there is one.

    python -m adam_amd.compare A B [-comparisons a,b,...|all] [-output_dir DIR]
"""
from __future__ import annotations

import argparse
import ctypes
import dataclasses
import os
import re
import sys
from collections import Counter, defaultdict
from typing import Dict, List, Optional, Tuple

from . import _capi
from ._capi import check, dblp, i32, pp, vp

CATS = ("unpairedPrimary", "pairedFirstPrimary", "pairedSecondPrimary", "unpairedSecondary", "pairedFirstSecondary",
        "pairedSecondSecondary", "unmapped")
# the categories BaseQualityScores.matchedByName visits (:172-177): not unpairedSecondary, not unmapped
BASEQ_CATS = ("unpairedPrimary", "pairedFirstPrimary", "pairedSecondPrimary", "pairedFirstSecondary",
              "pairedSecondSecondary")


def quality_scores(qual: str) -> List[int]:
    """RichADAMRecord.qualityScores: (char - 33).toByte, as Int."""
    out = []
    for ch in qual:
        v = (ord(ch) - 33) & 0xFF
        out.append(v - 256 if v >= 128 else v)
    return out


def load_buckets(path: str, encoding: str = "latin-1") -> Dict[str, List[Dict[str, List[List[int]]]]]:
    """readName -> its ReadBuckets (one per recordGroupId), each category a
    list of the reads' qualityScores in input order."""
    rg_names = set()
    body = []
    with open(path, "rb") as fh:
        for raw in fh.read().split(b"\n"):
            line = raw[:-1] if raw.endswith(b"\r") else raw
            if not line:
                continue
            if line.startswith(b"@"):
                f = line.split(b"\t")
                if f[0] == b"@RG":
                    for t in f[1:]:
                        if t.startswith(b"ID:"):
                            rg_names.add(t[3:])
                continue
            body.append(line)
    buckets: Dict[Tuple[Optional[bytes], bytes], Dict[str, List[List[int]]]] = {}
    for line in body:
        f = line.split(b"\t")
        name, flag, qual = f[0], int(f[1]), f[10]
        rg = None
        for t in f[11:]:
            k = t.split(b":", 2)
            if len(k) == 3 and k[0] == b"RG":
                rg = k[2]
        if rg is not None and rg not in rg_names:
            rg = None
        mapped = primary = paired = first = False
        if flag != 0:  # SAMRecordConverter.scala:72-108
            paired = bool(flag & 0x1)
            first = paired and bool(flag & 0x40)
            primary = not flag & 0x100
            mapped = not flag & 0x4
        b = buckets.setdefault((rg, name), {c: [] for c in CATS})
        q = quality_scores(qual.decode(encoding))
        if not mapped:
            cat = "unmapped"
        elif primary:
            cat = "pairedFirstPrimary" if first else ("pairedSecondPrimary" if paired else "unpairedPrimary")
        else:
            cat = "pairedFirstSecondary" if first else ("pairedSecondSecondary" if paired else "unpairedSecondary")
        b[cat].append(q)
    named: Dict[str, list] = defaultdict(list)
    for (rg, name), b in buckets.items():  # keyBy(_.allReads.head.getReadName)
        named[name.decode("latin-1")].append(b)
    return named


def base_quality_points(b1, b2) -> List[Tuple[int, int]]:
    """BaseQualityScores.matchedByName (AvailableComparisons.scala:149-177)."""
    pts: List[Tuple[int, int]] = []
    for c in BASEQ_CATS:
        r1, r2 = b1[c], b2[c]
        if len(r1) == len(r2) == 1:
            pts.extend(zip(r1[0], r2[0]))
    return pts


def compare_baseqs(path1: str, path2: str, encoding1: str = "latin-1", encoding2: str = "latin-1") -> dict:
    n1, n2 = load_buckets(path1, encoding1), load_buckets(path2, encoding2)
    hist: Counter = Counter()
    for name, bs1 in n1.items():  # named1.join(named2): every pair of buckets sharing the name
        for b1 in bs1:
            for b2 in n2.get(name, ()):
                hist.update(base_quality_points(b1, b2))
    count = sum(hist.values())
    identity = sum(v for (a, b), v in hist.items() if a == b)
    return dict(total1=sum(len(v) for v in n1.values()), unique1=sum(len(v) for k, v in n1.items() if k not in n2),
                total2=sum(len(v) for v in n2.values()), unique2=sum(len(v) for k, v in n2.items() if k not in n1),
                count=count, identity=identity, diff_pct=100.0 * (count - identity) / count if count else float("nan"),
                histogram=hist)


def summary(path1: str, path2: str, r: dict) -> str:
    """CompareAdam.printSummary's text."""
    out = ["%15s: %s" % ("INPUT1", path1), "\t%15s: %d" % ("total-reads", r["total1"]),
           "\t%15s: %d" % ("unique-reads", r["unique1"]), "%15s: %s" % ("INPUT2", path2),
           "\t%15s: %d" % ("total-reads", r["total2"]), "\t%15s: %d" % ("unique-reads", r["unique2"]), "",
           "baseqs", "\t%15s: %d" % ("count", r["count"]), "\t%15s: %d" % ("identity", r["identity"]),
           "\t%15s: %.5f" % ("diff%", r["diff_pct"])]
    return "\n".join(out)


# ---------------------------------------------------------------- all five ----
# The other comparisons of metrics/AvailableComparisons.scala:44-177, the
# filters of `findreads`, and the device path (csrc/compare.hip).  The names
# above stay as they were; everything below is new.

# DefaultComparisons.comparisons (AvailableComparisons.scala:27-32): name, description
COMPARISONS = (
    ("overmatched", "Checks that all buckets have exactly 0 or 1 records"),
    ("dupemismatch", "Counts the number of common reads marked as duplicates"),
    ("positions", "Counts how many reads align to the same genomic location"),
    ("mapqs", "Creates scatter plot of mapping quality scores across identical reads"),
    ("baseqs", "Creates scatter plots of base quality scores across identical positions in the same reads"),
)
COMPARISON_NAMES = tuple(n for n, _ in COMPARISONS)
KIND = {"overmatched": "boolean", "dupemismatch": "point", "positions": "long", "mapqs": "point", "baseqs": "point"}
VISITED = BASEQ_CATS  # every comparison visits these five categories


def find_comparison(name: str) -> str:
    """DefaultComparisons.findComparison"""
    if name not in COMPARISON_NAMES:
        raise ValueError("Could not find comparison %s" % name)
    return name


def parse_comparisons(names) -> Tuple[str, ...]:
    """CompareAdam.parseGenerators: a comma-separated list (or a sequence);
    ``all`` / None = the five in DefaultComparisons order."""
    if names is None or names == "all":
        return COMPARISON_NAMES
    if isinstance(names, str):
        names = names.split(",")
    return tuple(find_comparison(n) for n in names)


class CompareNullField(_capi.BQSRError):
    """NULL_FIELD of a comparison: where the reference unboxes a null.
    ``.side`` is 1 or 2, ``.read`` the read's ordinal in that input,
    ``.comparison`` the comparison that needed the field."""

    def __init__(self, comparison: str, side: int, read: int):
        field = {"positions": "start", "mapqs": "mapq", "baseqs": "qual"}[comparison]
        super().__init__(_capi.NULL_FIELD, "compare %s: read %d of input %d has a null %s (the reference throws a "
                         "NullPointerException)" % (comparison, read, side, field), read)
        self.comparison = comparison
        self.side = side


@dataclasses.dataclass
class Read:
    """The ADAMRecord fields the comparisons project (CompareAdam.setupTraversalEngine
    plus the comparisons' schemas).  quals: qualityScores, None for a null qual."""
    name: Optional[bytes] = None
    rg: Optional[object] = None
    mapped: bool = False
    primary: bool = False
    paired: bool = False
    first: bool = False
    dup: bool = False
    reference_id: Optional[int] = None
    reference_name: Optional[str] = None
    start: Optional[int] = None
    mapq: Optional[int] = None
    quals: Optional[List[int]] = None
    index: int = 0

    def category(self) -> str:
        if not self.mapped:
            return "unmapped"
        if self.primary:
            return "pairedFirstPrimary" if self.paired and self.first else (
                "pairedSecondPrimary" if self.paired else "unpairedPrimary")
        return "pairedFirstSecondary" if self.paired and self.first else (
            "pairedSecondSecondary" if self.paired else "unpairedSecondary")


class Bucket:
    """A ReadBucket: the reads of one (recordGroupId, readName) by category, input order kept."""

    def __init__(self, name, rg=None):
        self.name, self.rg = name, rg
        self.cats: Dict[str, List[Read]] = {c: [] for c in CATS}
        self.first = -1  # the ordinal of its first read

    def add(self, r: Read) -> None:
        if self.first < 0:
            self.first = r.index
        self.cats[r.category()].append(r)

    def all_reads(self) -> List[Read]:
        """ReadBucket.allReads (ReadBucket.scala:38-45)"""
        return [r for c in CATS for r in self.cats[c]]


def buckets_of(reads: List[Read]) -> List[Bucket]:
    """SingleReadBucket / ReadBucket of an input, in order of first appearance."""
    out: Dict[tuple, Bucket] = {}
    for r in reads:
        key = (r.rg, r.name)
        b = out.get(key)
        if b is None:
            b = out[key] = Bucket(r.name, r.rg)
        b.add(r)
    return list(out.values())


def java_chars(data: bytes, encoding: str = "latin-1") -> List[int]:
    """The low bytes of the Java chars of QUAL bytes: one per char; a code
    point above 0xFFFF (a 4-byte UTF-8 sequence) is a surrogate pair, two chars."""
    if encoding in ("latin-1", "latin1", "iso-8859-1"):
        return list(data)
    out = []
    for ch in data.decode(encoding):
        cp = ord(ch)
        if cp > 0xFFFF:
            v = cp - 0x10000
            out.append((0xD800 + (v >> 10)) & 0xFF)
            out.append((0xDC00 + (v & 0x3FF)) & 0xFF)
        else:
            out.append(cp & 0xFF)
    return out


def _scores(chars: List[int]) -> List[int]:
    out = []
    for c in chars:
        v = (c - 33) & 0xFF
        out.append(v - 256 if v >= 128 else v)
    return out


def read_sam_reads(path: str, encoding: str = "latin-1") -> List[Read]:
    """The records of a SAM file with SAMRecordConverter's semantics
    (converters/SAMRecordConverter.scala:26-108)."""
    sq: Dict[bytes, int] = {}
    rgs = set()
    reads: List[Read] = []
    with open(path, "rb") as fh:
        data = fh.read()
    for raw in data.split(b"\n"):
        line = raw[:-1] if raw.endswith(b"\r") else raw
        if not line:
            continue
        if line.startswith(b"@"):
            f = line.split(b"\t")
            for t in f[1:]:
                if f[0] == b"@SQ" and t.startswith(b"SN:"):
                    sq.setdefault(t[3:], len(sq))
                if f[0] == b"@RG" and t.startswith(b"ID:"):
                    rgs.add(t[3:])
            continue
        f = line.split(b"\t")
        flag = int(f[1])
        r = Read(name=f[0], index=len(reads))
        for t in f[11:]:
            k = t.split(b":", 2)
            if len(k) == 3 and k[0] == b"RG":
                r.rg = k[2]
        if r.rg is not None and r.rg not in rgs:
            r.rg = None
        if flag != 0:
            r.paired = bool(flag & 0x1)
            r.first = r.paired and bool(flag & 0x40)
            r.primary = not flag & 0x100
            r.mapped = not flag & 0x4
            r.dup = bool(flag & 0x400)
        if f[2] != b"*" and f[2] in sq:
            r.reference_id = sq[f[2]]
            r.reference_name = f[2].decode("latin-1")
            pos = int(f[3])
            if pos != 0:
                r.start = pos - 1
            try:
                mapq = int(f[4])
            except ValueError:
                mapq = 255
            if mapq != 255:
                r.mapq = mapq
        r.quals = _scores(java_chars(f[10], encoding))
        reads.append(r)
    return reads


# ---- the comparisons over a pair of buckets: the values, and the reads whose
# null field the reference would unbox as (side, read index) in `nulls`

def _single(b1: Bucket, b2: Bucket, c: str):
    r1, r2 = b1.cats[c], b2.cats[c]
    return (r1[0], r2[0]) if len(r1) == len(r2) == 1 else None


def overmatched(b1: Bucket, b2: Bucket, nulls=None) -> List[bool]:
    return [all(len(b1.cats[c]) == len(b2.cats[c]) and len(b1.cats[c]) <= 1 for c in VISITED)]


def dupemismatch(b1: Bucket, b2: Bucket, nulls=None) -> List[Tuple[int, int]]:
    return [(int(p[0].dup), int(p[1].dup)) for p in (_single(b1, b2, c) for c in VISITED) if p]


def positions(b1: Bucket, b2: Bucket, nulls=None) -> List[int]:
    total, bad = 0, False
    for c in VISITED:
        n1, n2 = len(b1.cats[c]), len(b2.cats[c])
        if n1 == n2 == 0:
            continue
        p = _single(b1, b2, c)
        if p is None or p[0].reference_id != p[1].reference_id:
            total -= 1  # the -1 sentinels add into the sum (AvailableComparisons.scala:110-115)
            continue
        for side, r in ((1, p[0]), (2, p[1])):
            if r.start is None:
                bad = True
                if nulls is None:
                    raise CompareNullField("positions", side, r.index)
                nulls.append((side, r.index))
        if not bad:
            total += abs(p[0].start - p[1].start)
    return [] if bad else [total]


def mapqs(b1: Bucket, b2: Bucket, nulls=None) -> List[Tuple[int, int]]:
    out = []
    for c in VISITED:
        p = _single(b1, b2, c)
        if not p:
            continue
        bad = False
        for side, r in ((1, p[0]), (2, p[1])):
            if r.mapq is None:
                bad = True
                if nulls is None:
                    raise CompareNullField("mapqs", side, r.index)
                nulls.append((side, r.index))
        if not bad:
            out.append((p[0].mapq, p[1].mapq))
    return out


def baseqs(b1: Bucket, b2: Bucket, nulls=None) -> List[Tuple[int, int]]:
    out: List[Tuple[int, int]] = []
    for c in VISITED:
        p = _single(b1, b2, c)
        if not p:
            continue
        bad = False
        for side, r in ((1, p[0]), (2, p[1])):
            if r.quals is None:
                bad = True
                if nulls is None:
                    raise CompareNullField("baseqs", side, r.index)
                nulls.append((side, r.index))
        if not bad:
            out.extend(zip(p[0].quals, p[1].quals))
    return out


GENERATORS = {"overmatched": overmatched, "dupemismatch": dupemismatch, "positions": positions, "mapqs": mapqs,
              "baseqs": baseqs}


# ---- util/Histogram.scala:28-59 over {key: count} dictionaries

def is_identical(key) -> bool:
    """Histogram.defaultFilter: equal pairs, 0, true"""
    if isinstance(key, tuple):
        return key[0] == key[1]
    if isinstance(key, bool):
        return key
    return key == 0


def hist_of(values) -> Dict[object, int]:
    return dict(Counter(values))


def hist_add(a: Dict[object, int], b: Dict[object, int]) -> Dict[object, int]:
    """Histogram.++"""
    out = dict(a)
    for k, v in b.items():
        out[k] = out.get(k, 0) + v
    return out


def hist_count(h: Dict[object, int]) -> int:
    return sum(h.values())


def hist_identical(h: Dict[object, int]) -> int:
    return sum(v for k, v in h.items() if is_identical(k))


@dataclasses.dataclass
class CompareResult:
    total1: int = 0
    unique1: int = 0
    total2: int = 0
    unique2: int = 0
    histograms: Dict[str, Dict[object, int]] = dataclasses.field(default_factory=dict)
    stats: Dict[str, object] = dataclasses.field(default_factory=dict, compare=False)


def joined(bs1: List[Bucket], bs2: List[Bucket]):
    """named1.join(named2) (ComparisonTraversalEngine.scala:45-59): every pair
    of buckets sharing the readName, ordered by bucket 1's first read, then
    bucket 2's; and the two unique counts."""
    n1: Dict[object, List[Bucket]] = defaultdict(list)
    n2: Dict[object, List[Bucket]] = defaultdict(list)
    for b in bs1:
        n1[b.name].append(b)
    for b in bs2:
        n2[b.name].append(b)
    pairs = [(b1, b2) for b1 in bs1 for b2 in n2.get(b1.name, ())]
    u1 = sum(1 for b in bs1 if b.name not in n2)
    u2 = sum(1 for b in bs2 if b.name not in n1)
    return pairs, u1, u2


def generate(bs1: List[Bucket], bs2: List[Bucket], comparisons):
    """engine.generate: [(bucket1, bucket2, {comparison: values})].  A null
    the reference would unbox raises CompareNullField: the first comparison in
    DefaultComparisons order that met one, side 1 before side 2, the first
    such read of that side in input order."""
    pairs, u1, u2 = joined(bs1, bs2)
    nulls = {c: [] for c in comparisons}
    rows = []
    for b1, b2 in pairs:
        rows.append((b1, b2, {c: GENERATORS[c](b1, b2, nulls[c]) for c in comparisons}))
    for c in COMPARISON_NAMES:
        for side in (1, 2):
            hit = [i for s, i in nulls.get(c, ()) if s == side]
            if hit:
                raise CompareNullField(c, side, min(hit))
    return rows, u1, u2


def compare_reads(reads1: List[Read], reads2: List[Read], comparisons=("baseqs",)) -> CompareResult:
    comparisons = parse_comparisons(comparisons)
    bs1, bs2 = buckets_of(reads1), buckets_of(reads2)
    rows, u1, u2 = generate(bs1, bs2, comparisons)
    hists = {c: Counter() for c in comparisons}
    for _, _, vals in rows:
        for c in comparisons:
            hists[c].update(vals[c])
    return CompareResult(len(bs1), u1, len(bs2), u2, {c: dict(h) for c, h in hists.items()})


def compare_host(path1: str, path2: str, comparisons=("baseqs",), encoding1: str = "latin-1",
                 encoding2: str = "latin-1") -> CompareResult:
    """All five comparisons in Python over two SAM text files: the path
    without a GPU, and the tests' oracle."""
    return compare_reads(read_sam_reads(path1, encoding1), read_sam_reads(path2, encoding2), comparisons)


def _need_sam_text(path1: str, path2: str) -> None:
    """the host path reads SAM text only"""
    if not _both_sam_text(path1, path2):
        raise ValueError("without a HIP device compare reads SAM text only; %s or %s is BAM or ADAM Parquet"
                         % (path1, path2))


def _have_device() -> bool:
    if not os.path.exists(_capi.LIB_PATH):
        return False
    try:
        import torch
        return bool(torch.cuda.is_available())
    except ImportError:
        return False


def compare(path1: str, path2: str, comparisons=("baseqs",), encoding1: str = "latin-1",
            encoding2: str = "latin-1") -> CompareResult:
    """compare_device when a HIP device is present, else compare_host."""
    if _have_device():
        return compare_device(path1, path2, comparisons, encoding1, encoding2)
    _need_sam_text(path1, path2)
    return compare_host(path1, path2, comparisons, encoding1, encoding2)


def summary_all(path1: str, path2: str, r: CompareResult, comparisons=None) -> str:
    """CompareAdam.printSummary's text for the comparisons, in order.  An
    empty histogram prints 0 and nan (the reference's reduce throws)."""
    comparisons = parse_comparisons(comparisons) if comparisons is not None else tuple(r.histograms)
    out = ["%15s: %s" % ("INPUT1", path1), "\t%15s: %d" % ("total-reads", r.total1),
           "\t%15s: %d" % ("unique-reads", r.unique1), "%15s: %s" % ("INPUT2", path2),
           "\t%15s: %d" % ("total-reads", r.total2), "\t%15s: %d" % ("unique-reads", r.unique2)]
    for c in comparisons:
        h = r.histograms[c]
        count, identity = hist_count(h), hist_identical(h)
        out += ["", c, "\t%15s: %d" % ("count", count), "\t%15s: %d" % ("identity", identity),
                "\t%15s: %.5f" % ("diff%", 100.0 * (count - identity) / count if count else float("nan"))]
    return "\n".join(out)


def format_key(key) -> str:
    """A histogram key as Scala's toString prints it"""
    if isinstance(key, bool):
        return "true" if key else "false"
    if isinstance(key, tuple):
        return "(%d,%d)" % key
    return "%d" % key


def histogram_text(h: Dict[object, int]) -> str:
    """Histogram.write, keys ascending"""
    return "value\tcount\n" + "".join("%s\t%d\n" % (format_key(k), h[k]) for k in sorted(h))


# ------------------------------------------------------------- findreads ----

POINT_RE = re.compile(r"\(\s*(-?\d+)\s*,\s*(-?\d+)\s*\)")  # BucketComparisons.pointRegex
FILTER_RE = re.compile(r"([^!=<>]+)((!=|=|<|>).*)")        # FindReads.filterRegex
_LEGAL = {"boolean": ("=",), "long": ("=", ">", "<"), "point": ("=", "!=")}


@dataclasses.dataclass(frozen=True)
class FilterTerm:
    comparison: str
    op: str
    value: object  # bool, int or (int, int)

    def passes(self, v) -> bool:
        if self.op == "=":
            return v == self.value
        if self.op == "!=":
            return v != self.value
        return v > self.value if self.op == ">" else v < self.value


def parse_filter(text: str) -> FilterTerm:
    """FindReads.parseFilter + the comparison's createFilter
    (metrics/Comparisons.scala:59-96,164-217); a refusal is a ValueError with
    the reference's message."""
    m = FILTER_RE.fullmatch(text)
    if not m:
        raise ValueError(text)
    name = find_comparison(m.group(1))
    op, value = m.group(3), m.group(2)[len(m.group(3)):]
    kind = KIND[name]
    if op not in _LEGAL[kind]:
        raise ValueError("\"%s\" isn't a legal filter value for %s" % (value, name))
    if kind == "boolean":
        if value.lower() not in ("true", "false"):
            raise ValueError('For input string: "%s"' % value)
        return FilterTerm(name, op, value.lower() == "true")
    if kind == "long":
        if not re.fullmatch(r"[+-]?\d+", value) or not -(1 << 63) <= int(value) < (1 << 63):
            raise ValueError('For input string: "%s"' % value)
        return FilterTerm(name, op, int(value))
    p = POINT_RE.fullmatch(value)
    if not p:
        raise ValueError("\"%s\" doesn't match point regex" % value)
    a, b = int(p.group(1)), int(p.group(2))
    for x in (a, b):
        if not -(1 << 31) <= x < (1 << 31):
            raise ValueError('For input string: "%d"' % x)
    return FilterTerm(name, op, (a, b))


def parse_filters(text: str) -> List[FilterTerm]:
    """FindReads.parseFilters: `;`-separated terms, a conjunction"""
    parts = text.split(";")
    while parts and parts[-1] == "":  # Java's split drops trailing empty strings
        parts.pop()
    return [parse_filter(t) for t in parts]


def combined_name(terms: List[FilterTerm]) -> str:
    """CombinedComparisons.name"""
    return "(%s)" % "+".join(t.comparison for t in terms)


def passes_filters(terms: List[FilterTerm], values: Dict[str, list]) -> bool:
    """CombinedFilter.passesFilter: every term met by some value of its comparison"""
    return all(any(t.passes(v) for v in values[t.comparison]) for t in terms)


def _position_text(ref_name, start) -> str:
    return "%s:%s" % ("null" if ref_name is None else ref_name, "null" if start is None else "%d" % start)


def find_reads_host(path1: str, path2: str, filters: str, encoding1: str = "latin-1",
                    encoding2: str = "latin-1") -> Tuple[str, List[Tuple[str, str, str]]]:
    """`findreads`: (the combined name, the rows (name, ref1:start1,
    ref2:start2) of the joined pairs that pass), rows ordered by bucket 1's
    first read, then bucket 2's."""
    terms = parse_filters(filters)
    comparisons = tuple(dict.fromkeys(t.comparison for t in terms))
    bs1 = buckets_of(read_sam_reads(path1, encoding1))
    bs2 = buckets_of(read_sam_reads(path2, encoding2))
    rows, _, _ = generate(bs1, bs2, comparisons)
    out = []
    for b1, b2, vals in rows:
        if passes_filters(terms, vals):
            h1, h2 = b1.all_reads()[0], b2.all_reads()[0]
            out.append((b1.name.decode("latin-1"), _position_text(h1.reference_name, h1.start),
                        _position_text(h2.reference_name, h2.start)))
    return combined_name(terms), out


def find_reads(path1: str, path2: str, filters: str, encoding1: str = "latin-1", encoding2: str = "latin-1"):
    if _have_device():
        return find_reads_device(path1, path2, filters, encoding1, encoding2)
    _need_sam_text(path1, path2)
    return find_reads_host(path1, path2, filters, encoding1, encoding2)


def find_reads_text(name: str, rows) -> str:
    return name + "\n" + "".join("\t".join(r) + "\n" for r in rows)


# ---------------------------------------------------------------- device ----

CMP_BIT = {n: 1 << i for i, n in enumerate(COMPARISON_NAMES)}
CMP_COLLISION = 1  # bqsr_compare_result.collision
_MAX_TERMS = 16
_OPS = {"=": 0, "!=": 1, "<": 2, ">": 3}


class _Options(ctypes.Structure):
    """bqsr_compare_options (include/adam_sam.h)"""
    _fields_ = [("hash_bits", ctypes.c_int32), ("utf8_1", ctypes.c_int32), ("utf8_2", ctypes.c_int32),
                ("comparisons", ctypes.c_uint32), ("flush_chars", ctypes.c_int64), ("baseq_groups", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class _Term(ctypes.Structure):
    """bqsr_compare_term"""
    _fields_ = [("comparison", ctypes.c_int32), ("op", ctypes.c_int32), ("a", ctypes.c_int64), ("b", ctypes.c_int64)]


class _Result(ctypes.Structure):
    """bqsr_compare_result"""
    _fields_ = [("total1", ctypes.c_int64), ("unique1", ctypes.c_int64), ("total2", ctypes.c_int64),
                ("unique2", ctypes.c_int64), ("n_pairs", ctypes.c_int64), ("overmatched", ctypes.c_int64 * 2),
                ("dupemismatch", ctypes.c_int64 * 4), ("n_positions", ctypes.c_int64), ("n_mapqs", ctypes.c_int64),
                ("n_rows", ctypes.c_int64), ("collision", ctypes.c_int32),
                ("null_comparison", ctypes.c_int32), ("null_side", ctypes.c_int32), ("flushes", ctypes.c_int32),
                ("null_read", ctypes.c_int64), ("baseq_chars", ctypes.c_int64)]


class _Side(ctypes.Structure):
    """bqsr_compare_side"""
    _fields_ = [("sam", ctypes.c_void_p), ("arrow", ctypes.c_void_p), ("chunk_reads", ctypes.POINTER(ctypes.c_int64)),
                ("first_of_pair", ctypes.POINTER(ctypes.c_void_p)),
                ("first_of_pair_validity", ctypes.POINTER(ctypes.c_void_p)),
                ("mapq", ctypes.POINTER(ctypes.c_void_p)), ("mapq_validity", ctypes.POINTER(ctypes.c_void_p)),
                ("n_chunks", ctypes.c_int32)]


KERNELS = ("join", "scalar", "baseqs")
_SIG = {
    "bqsr_compare_create": (ctypes.c_int, [vp, ctypes.POINTER(_Options), pp]),
    "bqsr_compare_destroy": (None, [vp]),
    "bqsr_compare_sides": (ctypes.c_int, [vp, ctypes.POINTER(_Side), ctypes.POINTER(_Side), ctypes.POINTER(_Term), i32,
                                          vp, ctypes.POINTER(_Result)]),
    "bqsr_compare_values": (ctypes.c_int, [vp, i32, vp, vp]),
    "bqsr_compare_baseqs": (ctypes.c_int, [vp, vp]),
    "bqsr_compare_rows": (ctypes.c_int, [vp, vp, vp]),
    "bqsr_compare_kernel_times": (ctypes.c_int, [vp, dblp, dblp, dblp]),
}


def _lib():
    return _capi.bind(_capi.lib(), _SIG)


def _kernel_times(h) -> Tuple[float, float, float]:
    """(join, scalar, baseqs + UTF-8 decode) kernel milliseconds of the handle's last run (measurement only)"""
    return tuple(_capi.stage_times(_lib().bqsr_compare_kernel_times, KERNELS, handle=h).values())


def _is_utf8(encoding: str) -> int:
    e = encoding.lower().replace("_", "-")
    if e in ("latin-1", "latin1", "iso-8859-1"):
        return 0
    if e in ("utf-8", "utf8"):
        return 1
    raise ValueError("the device path reads QUAL bytes as latin-1 or utf-8, not %s" % encoding)


# CompareAdam.setupTraversalEngine's projection, and each comparison's `schemas`
ENGINE_COLUMNS = ("recordGroupId", "readName", "readMapped", "primaryAlignment", "readPaired", "firstOfPair")
SCHEMAS = {"overmatched": (), "dupemismatch": ("duplicateRead",), "positions": ("referenceId", "start", "firstOfPair"),
           "mapqs": ("mapq",), "baseqs": ("qual",)}


class _SamSide:
    """one input as a bqsr_sam parse (SAM text or BAM)"""

    def __init__(self, path: str, ctx):
        from .sam import SamText
        self.sam = SamText.read(path, ctx)
        self.n_reads = self.sam.counts().n_reads
        self._lines = self._known = None

    def struct(self) -> _Side:
        return _Side(sam=self.sam.h)

    def row(self, i: int) -> Tuple[str, str]:
        """(readName, ref:start) of read i, as the parse read them: referenceName is set exactly for
        the RNAMEs the parse resolved (SamText.ref_names), start for a resolved RNAME and POS != 0"""
        if self._lines is None:
            self._lines = [ln for ln in (raw[:-1] if raw.endswith(b"\r") else raw for raw in self.sam.text().split(b"\n"))
                           if ln and not ln.startswith(b"@")]
            self._known = {n.encode("latin-1") for n in self.sam.ref_names()}
        f = self._lines[i].split(b"\t", 5)
        if f[2] not in self._known:
            return f[0].decode("latin-1"), "null:null"
        pos = int(f[3])
        return f[0].decode("latin-1"), _position_text(f[2].decode("latin-1"), pos - 1 if pos != 0 else None)

    def close(self):
        self.sam.close()


class _ArrowSide:
    """one input as ADAMRecord Parquet (a file or a directory of part files): Arrow reads the
    projected columns on the host, bqsr_arrow_load puts them on the device; firstOfPair and mapq,
    which bqsr_arrow_chunk does not carry, go to the compare call as per-chunk buffers"""

    def __init__(self, path: str, ctx, comparisons, rows: bool):
        from . import parquet as P
        pa = P._pa()[0]
        cols = list(ENGINE_COLUMNS)
        for c in comparisons:
            cols += [x for x in SCHEMAS[c] if x not in cols]
        if rows:  # findreads prints allReads.head's referenceName and start
            cols += [x for x in ("referenceName", "start") if x not in cols]
        self.table = P.read_table(path, columns=cols)
        self.reads = P.ArrowReads(self.table, ctx, markdup=True)
        self.n_reads = self.table.num_rows
        names = set(self.table.column_names)
        self.keep = []
        sizes, fp, fpv, mq, mqv = [], [], [], [], []

        def buffers(rb, name, typ):
            a = rb.column(rb.schema.get_field_index(name))
            if a.type != typ:
                a = a.cast(typ)
            if a.offset:
                a = pa.concat_arrays([a])
            self.keep.append(a)
            b = a.buffers()
            return (b[1].address if b[1] is not None else None), (b[0].address if b[0] is not None else None)

        for rb in self.table.to_batches():
            if rb.num_rows == 0:
                continue
            sizes.append(rb.num_rows)
            d, v = buffers(rb, "firstOfPair", pa.bool_()) if "firstOfPair" in names else (None, None)
            fp.append(d)
            fpv.append(v)
            d, v = buffers(rb, "mapq", pa.int32()) if "mapq" in names else (None, None)
            mq.append(d)
            mqv.append(v)
        k = len(sizes)
        self._c = ((ctypes.c_int64 * max(1, k))(*sizes), (ctypes.c_void_p * max(1, k))(*fp),
                   (ctypes.c_void_p * max(1, k))(*fpv), (ctypes.c_void_p * max(1, k))(*mq),
                   (ctypes.c_void_p * max(1, k))(*mqv))
        self._k = k

    def struct(self) -> _Side:
        c = self._c
        return _Side(arrow=self.reads.h, chunk_reads=c[0], first_of_pair=c[1], first_of_pair_validity=c[2], mapq=c[3],
                     mapq_validity=c[4], n_chunks=self._k)

    def row(self, i: int) -> Tuple[str, str]:
        def at(name):
            return self.table.column(name)[int(i)].as_py() if name in self.table.column_names else None
        name = at("readName")
        return ("null" if name is None else name), _position_text(at("referenceName"), at("start"))

    def close(self):
        self.reads.close()


def _open_side(path: str, ctx, comparisons=(), rows: bool = False):
    from .transform import is_parquet
    return _ArrowSide(path, ctx, comparisons, rows) if is_parquet(path) else _SamSide(path, ctx)


def _device_run(path1, path2, comparisons, encoding1, encoding2, terms, _hash_bits, _flush_chars, _groups=0):
    import numpy as np

    from . import bqsr
    L = _lib()
    ctx = bqsr.Context.get(0)
    opt = _Options(hash_bits=_hash_bits, utf8_1=_is_utf8(encoding1), utf8_2=_is_utf8(encoding2),
                   comparisons=sum(CMP_BIT[c] for c in comparisons), flush_chars=_flush_chars,
                   baseq_groups=_groups)
    h = ctypes.c_void_p()
    s1 = s2 = None
    try:
        s1 = _open_side(path1, ctx, comparisons, bool(terms))
        s2 = _open_side(path2, ctx, comparisons, bool(terms))
        check(L.bqsr_compare_create(ctx.handle, ctypes.byref(opt), ctypes.byref(h)))
        arr = (_Term * max(1, len(terms)))()
        for k, t in enumerate(terms):
            v = t.value
            a, b = (v if isinstance(v, tuple) else (int(v), 0))
            arr[k] = _Term(COMPARISON_NAMES.index(t.comparison), _OPS[t.op], a, b)
        res = _Result()
        d1, d2 = s1.struct(), s2.struct()
        st = L.bqsr_compare_sides(h, ctypes.byref(d1), ctypes.byref(d2), arr, len(terms), None, ctypes.byref(res))
        if st == _capi.NULL_FIELD and res.null_side:
            raise CompareNullField(COMPARISON_NAMES[res.null_comparison], res.null_side, res.null_read)
        check(st)
        if res.collision:
            return None, None, res
        out = CompareResult(res.total1, res.unique1, res.total2, res.unique2)
        out.stats = dict(pairs=res.n_pairs, flushes=res.flushes, baseq_chars=res.baseq_chars,
                         reads=s1.n_reads + s2.n_reads, kernel_ms=_kernel_times(h))
        for c in comparisons:
            if c == "overmatched":
                hist = {k: res.overmatched[int(k)] for k in (False, True) if res.overmatched[int(k)]}
            elif c == "dupemismatch":
                hist = {(a, b): res.dupemismatch[2 * a + b] for a in (0, 1) for b in (0, 1)
                        if res.dupemismatch[2 * a + b]}
            elif c == "positions":
                v, n = np.zeros(res.n_positions, np.int64), np.zeros(res.n_positions, np.int64)
                check(L.bqsr_compare_values(h, 2, v.ctypes.data, n.ctypes.data))
                hist = {int(x): int(y) for x, y in zip(v, n)}
            elif c == "mapqs":
                v, n = np.zeros(res.n_mapqs, np.uint64), np.zeros(res.n_mapqs, np.int64)
                check(L.bqsr_compare_values(h, 3, v.ctypes.data, n.ctypes.data))
                m1 = (v >> np.uint64(32)).astype(np.uint32).view(np.int32)
                m2 = (v & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
                hist = {(int(a), int(b)): int(y) for a, b, y in zip(m1, m2, n)}
            else:
                t = np.zeros((256, 256), np.int64)
                check(L.bqsr_compare_baseqs(h, t.ctypes.data))
                hist = {}
                for a, b in zip(*np.nonzero(t)):  # indexed by the low bytes; a score is a signed byte
                    hist[(int(a) - 256 if a >= 128 else int(a), int(b) - 256 if b >= 128 else int(b))] = int(t[a, b])
            out.histograms[c] = hist
        rows = None
        if terms:
            r1, r2 = np.zeros(res.n_rows, np.uint32), np.zeros(res.n_rows, np.uint32)
            check(L.bqsr_compare_rows(h, r1.ctypes.data, r2.ctypes.data))
            rows = []
            for a, b in zip(r1, r2):
                (name, pos1), (_, pos2) = s1.row(int(a)), s2.row(int(b))
                rows.append((name, pos1, pos2))
        return out, rows, res
    finally:
        if h:
            L.bqsr_compare_destroy(h)
        for s in (s1, s2):
            if s is not None:
                s.close()


def _both_sam_text(path1: str, path2: str) -> bool:
    from .transform import is_parquet
    for p in (path1, path2):
        if is_parquet(p):
            return False
        with open(p, "rb") as fh:
            if fh.read(4) == b"\x1f\x8b\x08\x04":
                return False
    return True


_COLLISION = ("compare: two (recordGroupId, readName) keys of one input share a %d-bit hash; the host path "
              "decides for SAM text only")


def compare_device(path1: str, path2: str, comparisons=("baseqs",), encoding1: str = "latin-1",
                   encoding2: str = "latin-1", _hash_bits: int = 64, _flush_chars: int = 0,
                   _groups: int = 0) -> CompareResult:
    """The comparisons on the device (csrc/compare.hip) over SAM, BAM or
    ADAM Parquet inputs (a file or a part-file directory, read with
    CompareAdam's projection plus the comparisons' schemas; its qual is
    always UTF-8, whatever ``encoding`` says), each one partition.  A hash collision inside one input's
    bucketing is reported by the library; SAM text then goes through
    compare_host, any other input raises UNSUPPORTED."""
    comparisons = parse_comparisons(comparisons)
    out, _, res = _device_run(path1, path2, comparisons, encoding1, encoding2, [], _hash_bits, _flush_chars, _groups)
    if out is None:
        if not _both_sam_text(path1, path2):
            raise _capi.BQSRError(_capi.UNSUPPORTED, _COLLISION % _hash_bits)
        out = compare_host(path1, path2, comparisons, encoding1, encoding2)
        out.stats = dict(fallback="host")
    return out


def find_reads_device(path1: str, path2: str, filters: str, encoding1: str = "latin-1", encoding2: str = "latin-1",
                      _hash_bits: int = 64, _flush_chars: int = 0):
    terms = parse_filters(filters)
    if len(terms) > _MAX_TERMS:
        raise _capi.BQSRError(_capi.UNSUPPORTED, "findreads on the device takes at most %d terms" % _MAX_TERMS)
    comparisons = tuple(c for c in COMPARISON_NAMES if any(t.comparison == c for t in terms))
    out, rows, res = _device_run(path1, path2, comparisons, encoding1, encoding2, terms, _hash_bits, _flush_chars)
    if out is None:
        if not _both_sam_text(path1, path2):
            raise _capi.BQSRError(_capi.UNSUPPORTED, _COLLISION % _hash_bits)
        return find_reads_host(path1, path2, filters, encoding1, encoding2)
    return combined_name(terms), rows


# ------------------------------------------------------------------- CLI ----

def list_comparisons_text() -> str:
    return "\nAvailable comparisons:\n" + "".join("\t%10s : %s\n" % c for c in COMPARISONS)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="adam_amd.compare", description="compare two read sets (SAM, BAM, ADAM Parquet)")
    ap.add_argument("input1", nargs="?")
    ap.add_argument("input2", nargs="?")
    ap.add_argument("-comparisons", default="baseqs", help="a,b,...|all; see -list_comparisons")
    ap.add_argument("-list_comparisons", action="store_true")
    ap.add_argument("-encoding1", default="latin-1")
    ap.add_argument("-encoding2", default="latin-1")
    ap.add_argument("-output", default=None, help="also write the histogram (value\\tcount) of the one comparison here")
    ap.add_argument("-output_dir", default=None, help="write files, summary.txt and a histogram per comparison here")
    ap.add_argument("-recurse1", default=None)
    ap.add_argument("-recurse2", default=None)
    a = ap.parse_args(argv)
    if a.list_comparisons:
        sys.stdout.write(list_comparisons_text())
        return 0
    if a.recurse1 is not None or a.recurse2 is not None:
        ap.error("-recurse1 / -recurse2 are not in this build: each input is one file (or one part-file directory)")
    if a.input1 is None or a.input2 is None:
        ap.error("INPUT1 and INPUT2 are required")
    comparisons = parse_comparisons(a.comparisons)
    if a.output and len(comparisons) != 1:
        ap.error("-output takes exactly one comparison; use -output_dir")
    r = compare(a.input1, a.input2, comparisons, a.encoding1, a.encoding2)
    text = summary_all(a.input1, a.input2, r, comparisons)
    if a.output_dir:
        os.makedirs(a.output_dir, exist_ok=True)
        with open(os.path.join(a.output_dir, "files"), "w") as fh:
            fh.write(a.input1 + "\n" + a.input2 + "\n")
        with open(os.path.join(a.output_dir, "summary.txt"), "w") as fh:
            fh.write(text + "\n")
        for c in comparisons:
            with open(os.path.join(a.output_dir, c), "w") as fh:
                fh.write(histogram_text(r.histograms[c]))
    else:
        print(text)
    if a.output:
        with open(a.output, "w") as fh:  # Histogram.write
            fh.write(histogram_text(r.histograms[comparisons[0]]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
