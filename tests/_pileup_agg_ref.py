"""PileupAggregator restated in plain Python: the yardstick of the aggregation
tests.

``flatten`` and ``aggregate`` of adam-core/.../rdd/PileupAggregator.scala:25-219,
written from the Scala over the row dicts ``_pileup_ref`` produces (a missing
key or None is a null field), with Java's int arithmetic made explicit.  The
reference leaves two orders to Spark; the ones include/adam_sam.h declares are
used here: rows fold in the order given, groups come out ascending by
(referenceId, position, readBase ordinal, rangeOffset, recordGroupSample bytes),
nulls first in every component.  Nothing here knows how the device does it.

Where the Scala throws, :class:`AggThrow` carries the C ABI's status name and
the offending input row: first what throws while grouping (a null referenceId
or position, NULL_FIELD), then what the folds throw (NULL_FIELD for a null
mapQuality, sangerQuality or countAtPosition in any row and for a null
numSoftClipped, numReverseStrand, readStart or readEnd in a group of two or
more; PILEUP for a division by a zero count, at the group's first row); in
either stage the lowest row decides, NULL_FIELD before PILEUP on one row.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

from _pileup_ref import BASES, FIELDS

STRING_RG = ["recordGroupSequencingCenter", "recordGroupDescription", "recordGroupFlowOrder",
             "recordGroupKeySequence", "recordGroupLibrary", "recordGroupPlatform", "recordGroupPlatformUnit",
             "recordGroupSample"]
NUMBER_RG = ["recordGroupRunDateEpoch", "recordGroupPredictedMedianInsertSize"]


class AggThrow(Exception):
    def __init__(self, status: str, row: int = -1, what: str = ""):
        super().__init__("%s: row %d %s" % (status, row, what))
        self.status = status
        self.row = row


def i32(x: int) -> int:
    """a Java int: wrapped to 32 bits, signed"""
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= 1 << 31 else x


def java_div(a: int, b: int) -> int:
    """Java's int division: toward zero; Int.MinValue / -1 = Int.MinValue"""
    if b == 0:
        raise ZeroDivisionError
    q = abs(a) // abs(b)
    return i32(q if (a < 0) == (b < 0) else -q)


def fold_string(v: Optional[str], w: Optional[str]) -> Optional[str]:
    """List(Option(a), Option(b)).flatten.distinct joined with ","; none: unset"""
    vals = [x for x in (v, w) if x is not None]
    distinct = []
    for x in vals:
        if x not in distinct:
            distinct.append(x)
    return ",".join(distinct) if distinct else None


def fold_number(v, w):
    """set only when exactly one distinct non-null value is among (a, b)"""
    distinct = {x for x in (v, w) if x is not None}
    return distinct.pop() if len(distinct) == 1 else None


def _name(v) -> str:
    return "null" if v is None else v  # Java's string concatenation


def _unbox(row, field):
    if row.get(field) is None:
        raise AggThrow("NULL_FIELD", -1, field)
    return row[field]


def reduce_step(a: dict, b: dict, names: bool = True) -> dict:
    """the function combineEvidence reduces with (validate = false); names
    False: readName is left to the caller (see aggregate_pileup)"""
    c = dict.fromkeys(FIELDS)
    for f in ("referenceName", "referenceId", "position", "rangeOffset", "rangeLength", "referenceBase", "readBase"):
        c[f] = a.get(f)
    for f in STRING_RG:
        c[f] = fold_string(a.get(f), b.get(f))
    for f in NUMBER_RG:
        c[f] = fold_number(a.get(f), b.get(f))
    u = _unbox
    c["mapQuality"] = i32(u(a, "mapQuality") * u(a, "countAtPosition") + u(b, "mapQuality") * u(b, "countAtPosition"))
    c["sangerQuality"] = i32(u(a, "sangerQuality") * u(a, "countAtPosition") +
                             u(b, "sangerQuality") * u(b, "countAtPosition"))
    c["countAtPosition"] = i32(a["countAtPosition"] + b["countAtPosition"])
    c["numSoftClipped"] = i32(u(a, "numSoftClipped") + u(b, "numSoftClipped"))
    c["numReverseStrand"] = i32(u(a, "numReverseStrand") + u(b, "numReverseStrand"))
    if names:
        c["readName"] = _name(a.get("readName")) + "," + _name(b.get("readName"))
    c["readStart"] = min(u(a, "readStart"), u(b, "readStart"))
    c["readEnd"] = max(u(a, "readEnd"), u(b, "readEnd"))
    return c


def aggregate_pileup(rows: List[dict]) -> dict:
    """aggregatePileup: reduce (a left fold; one row: the row itself), then
    the two divisions"""
    acc = dict(rows[0])
    for b in rows[1:]:
        acc = reduce_step(acc, b, names=False)
    if len(rows) > 1:  # the left fold of a + "," + b, joined once (a deep group's fold is quadratic otherwise)
        acc["readName"] = ",".join(_name(r.get("readName")) for r in rows)
    num = _unbox(acc, "countAtPosition")
    mq, sq = _unbox(acc, "mapQuality"), _unbox(acc, "sangerQuality")
    acc["mapQuality"] = java_div(mq, num)
    acc["sangerQuality"] = java_div(sq, num)
    return acc


def minor_key(row: dict) -> Tuple:
    """mapPileup's key in the declared order: nulls first"""
    g = row.get
    rb, ro, sm = g("readBase"), g("rangeOffset"), g("recordGroupSample")
    return ((0, 0) if rb is None else (1, BASES.index(rb)), (0, 0) if ro is None else (1, ro),
            (0, b"") if sm is None else (1, sm.encode()))


def _fold_errors(rows: List[dict], index: List[int]) -> List[Tuple[int, int, str]]:
    """(row, order, status) of everything folding this group would throw"""
    out = []
    for r, i in zip(rows, index):
        if any(r.get(f) is None for f in ("mapQuality", "sangerQuality", "countAtPosition")):
            out.append((i, 0, "NULL_FIELD"))
        elif len(rows) > 1 and any(r.get(f) is None for f in ("numSoftClipped", "numReverseStrand", "readStart",
                                                              "readEnd")):
            out.append((i, 0, "NULL_FIELD"))
    if not out and i32(sum(r["countAtPosition"] for r in rows)) == 0:
        out.append((index[0], 1, "PILEUP"))
    return out


def _groups(rows: List[dict], index: List[int], key) -> List[Tuple[Tuple, List[dict], List[int]]]:
    seen: Dict[Tuple, Tuple[List[dict], List[int]]] = {}
    for r, i in zip(rows, index):
        g = seen.setdefault(key(r), ([], []))
        g[0].append(r)
        g[1].append(i)
    return [(k,) + seen[k] for k in sorted(seen)]


def flatten(rows: List[dict], index: Optional[List[int]] = None) -> List[dict]:
    """flatten(kv): the rows of one position, grouped by mapPileup's key and
    aggregated; groups in the declared order"""
    index = list(range(len(rows))) if index is None else index
    groups = _groups(rows, index, minor_key)
    errors = [e for _, g, ix in groups for e in _fold_errors(g, ix)]
    if errors:
        row, _, status = min(errors)
        raise AggThrow(status, row)
    return [aggregate_pileup(g) for _, g, _ in groups]


def aggregate(rows: List[dict]) -> List[dict]:
    """aggregate(pileups): groupBy ReferencePosition, flatten every position;
    positions ascending by (referenceId, position)"""
    for i, r in enumerate(rows):
        if r.get("referenceId") is None or r.get("position") is None:
            raise AggThrow("NULL_FIELD", i, "ReferencePosition")
    positions = _groups(rows, list(range(len(rows))), lambda r: (r["referenceId"], r["position"]))
    errors = []
    for _, g, ix in positions:
        for _, gg, iix in _groups(g, ix, minor_key):
            errors += _fold_errors(gg, iix)
    if errors:
        row, _, status = min(errors)
        raise AggThrow(status, row)
    out: List[dict] = []
    for _, g, ix in positions:
        out += flatten(g, ix)
    return out
