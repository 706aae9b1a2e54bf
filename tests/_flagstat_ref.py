"""A restatement of the reference's flagstat over the ADAMRecord dicts
``_adam_ref.convert_sam`` returns (None = null):

  adamFlagStat   adam-core/.../rdd/FlagStat.scala:21-116
  the command    adam-cli/.../cli/FlagStat.scala:43-109 (percent: :63, the text: :65-108)

Independent of adam_amd/flagstat.py (plain Python over dicts, fractions for
the rounding)."""
from __future__ import annotations

import struct
from fractions import Fraction
from typing import List, Sequence, Tuple

# FlagStatMetrics' fields, DuplicateMetrics flattened (rdd/FlagStat.scala:49-62)
NAMES = ("total",
         "duplicatesPrimary.total", "duplicatesPrimary.bothMapped", "duplicatesPrimary.onlyReadMapped",
         "duplicatesPrimary.crossChromosome",
         "duplicatesSecondary.total", "duplicatesSecondary.bothMapped", "duplicatesSecondary.onlyReadMapped",
         "duplicatesSecondary.crossChromosome",
         "mapped", "pairedInSequencing", "read1", "read2", "properlyPaired", "withSelfAndMateMapped", "singleton",
         "withMateMappedToDiffChromosome", "withMateMappedToDiffChromosomeMapQ5")


class NullMapq(Exception):
    """`p.getMapq >= 5` unboxing a null (rdd/FlagStat.scala:100): .read = the record's index"""

    def __init__(self, read: int):
        super().__init__("read %d: NullPointerException (mapq)" % read)
        self.read = read


def _ne(a, b) -> bool:
    """Scala's != on boxed Integers (rdd/FlagStat.scala:43,88): equals(),
    null equal to null only"""
    if a is None or b is None:
        return not (a is None and b is None)
    return int(a) != int(b)


def record_metrics(p: dict, index: int = 0) -> Tuple[List[int], bool]:
    """one record's FlagStatMetrics (rdd/FlagStat.scala:87-101) and its failedQuality"""
    diff = p["readPaired"] and p["readMapped"] and p["mateMapped"] and _ne(p["referenceId"], p["mateReferenceId"])

    def dup(f: bool) -> List[int]:  # :39-44 -- not gated by readPaired
        return [int(f), int(f and p["readMapped"] and p["mateMapped"]),
                int(f and p["readMapped"] and not p["mateMapped"]),
                int(f and _ne(p["referenceId"], p["mateReferenceId"]))]
    primary = dup(p["duplicateRead"] and p["primaryAlignment"])        # :32-34
    secondary = dup(p["duplicateRead"] and not p["primaryAlignment"])  # :35-37
    if diff and p["mapq"] is None:  # :100: && evaluates getMapq only when diff holds
        raise NullMapq(index)
    m = [1] + primary + secondary + [
        int(p["readMapped"]),
        int(p["readPaired"]),
        int(p["readPaired"] and p["firstOfPair"]),
        int(p["readPaired"] and p["secondOfPair"]),
        int(p["readPaired"] and p["properPair"]),
        int(p["readPaired"] and p["readMapped"] and p["mateMapped"]),
        int(p["readPaired"] and p["readMapped"] and not p["mateMapped"]),
        int(diff),
        int(diff and p["mapq"] >= 5)]
    return m, bool(p["failedVendorQualityChecks"])


def throws(p: dict) -> bool:
    try:
        record_metrics(p)
    except NullMapq:
        return True
    return False


def flagstat_ref(recs: Sequence[dict]) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    """(failed, passed) -- the aggregate's order (rdd/FlagStat.scala:102-114);
    raises NullMapq at the first record that throws"""
    failed, passed = [0] * 18, [0] * 18
    for i, p in enumerate(recs):
        m, f = record_metrics(p, i)
        acc = failed if f else passed
        for k in range(18):
            acc[k] += m[k]
    return tuple(failed), tuple(passed)


def percent_ref(fraction: int, total: int) -> float:
    """cli/FlagStat.scala:63: `100.00 * fraction.toFloat / total`, 0.0 for an
    empty total; toFloat: the nearest 32-bit float"""
    if total == 0:
        return 0.0
    as_float = struct.unpack("<f", struct.pack("<f", float(fraction)))[0]
    return 100.00 * as_float / total


def java_2f_ref(x: float) -> str:
    """Java's %.2f: Double.toString's (shortest round-tripping) digits,
    rounded half up at the second place"""
    q = Fraction(repr(float(x))) * 100 + Fraction(1, 2)
    cents = q.numerator // q.denominator  # floor: x >= 0 here
    return "%d.%02d" % divmod(cents, 100)


_WORDS = ("in total (QC-passed reads + QC-failed reads)",
          "primary duplicates",
          "primary duplicates - both read and mate mapped",
          "primary duplicates - only read mapped",
          "primary duplicates - cross chromosome",
          "secondary duplicates",
          "secondary duplicates - both read and mate mapped",
          "secondary duplicates - only read mapped",
          "secondary duplicates - cross chromosome",
          "mapped", "paired in sequencing", "read1", "read2", "properly paired", "with itself and mate mapped",
          "singletons", "with mate mapped to a different chr", "with mate mapped to a different chr (mapQ>=5)")
_PERCENT = (9, 13, 15)  # mapped, properly paired, singletons (cli/FlagStat.scala:75,79,81)


def format_ref(failed: Sequence[int], passed: Sequence[int]) -> str:
    """what cli/FlagStat.scala:65-108 gives println: the stripMargin'd string
    opens with a line break and ends with the closing quotes' line of
    thirteen spaces"""
    s = "\n"
    for k in range(18):
        s += "%d + %d %s" % (passed[k], failed[k], _WORDS[k])
        if k in _PERCENT:
            s += " (%s%%:%s%%)" % (java_2f_ref(percent_ref(passed[k], passed[0])),
                                   java_2f_ref(percent_ref(failed[k], failed[0])))
        s += "\n"
    return s + " " * 13
