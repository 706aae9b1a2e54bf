"""`adam flagstat`: per-flag read statistics on the device
(adam-cli/.../cli/FlagStat.scala:43-109 over adamFlagStat,
adam-core/.../rdd/FlagStat.scala:21-116).

    python -m adam_amd.flagstat INPUT.{sam,bam,adam,parquet} [-partition_bytes N]

prints the reference's text on stdout and a ``reads=... phases=...`` line on
stderr.  SAM text streams through the device in ``inputs.sam_partitions``
partitions, each parsed with the header, counted (bqsr_sam_flagstat) and
closed; the counts are integer sums, so any number of partitions gives the
same result.  A BAM is one parse.  ADAMRecord Parquet is read by Arrow with
the command's projection (only the columns the file has; a missing one is
passed as NULL) and every record batch's buffers go to the device as they are
(bqsr_flagstat_arrow).

A read whose mate is mapped to a different chromosome while its mapq is null
makes the reference throw (it unboxes null): ``BQSRError`` NULL_FIELD, whose
``.read`` is the read's ordinal in the whole input.
"""
from __future__ import annotations

import argparse
import ctypes
import dataclasses
import decimal
import struct
import sys
import time
from typing import Dict, Optional, Tuple

from . import _capi, bqsr
from ._capi import check, i32, vp
from .inputs import DEFAULT_PARTITION_BYTES, Phases, SamInput, add_region_arguments, is_parquet, rebased, region_plan, report

# the command's projection (cli/FlagStat.scala:50-57), booleans in bqsr_flagstat_chunk's order
BOOL_COLUMNS = ("readPaired", "properPair", "readMapped", "mateMapped", "firstOfPair", "secondOfPair",
                "primaryAlignment", "duplicateRead", "failedVendorQualityChecks")
INT_COLUMNS = ("referenceId", "mateReferenceId", "mapq")
PROJECTION = BOOL_COLUMNS + INT_COLUMNS


@dataclasses.dataclass(frozen=True)
class FlagStatMetrics:
    """The eighteen counts of one side (passed or failed) in the reference's
    order: FlagStatMetrics' fields, DuplicateMetrics flattened (rdd/FlagStat.scala:49-62)."""
    total: int = 0
    dup_primary_total: int = 0
    dup_primary_both_mapped: int = 0
    dup_primary_only_read_mapped: int = 0
    dup_primary_cross_chromosome: int = 0
    dup_secondary_total: int = 0
    dup_secondary_both_mapped: int = 0
    dup_secondary_only_read_mapped: int = 0
    dup_secondary_cross_chromosome: int = 0
    mapped: int = 0
    paired_in_sequencing: int = 0
    read1: int = 0
    read2: int = 0
    properly_paired: int = 0
    with_self_and_mate_mapped: int = 0
    singleton: int = 0
    with_mate_mapped_to_diff_chromosome: int = 0
    with_mate_mapped_to_diff_chromosome_mapq5: int = 0

    def counts(self) -> Tuple[int, ...]:
        return dataclasses.astuple(self)

    def __add__(self, that: "FlagStatMetrics") -> "FlagStatMetrics":
        return FlagStatMetrics(*[a + b for a, b in zip(self.counts(), that.counts())])


class _Metrics(ctypes.Structure):
    _fields_ = [("c", ctypes.c_int64 * 18)]


class _FlagStat(ctypes.Structure):
    _fields_ = [("passed", _Metrics), ("failed", _Metrics)]


class FlagStatChunk(ctypes.Structure):
    """bqsr_flagstat_chunk (include/adam_sam.h)"""
    _fields_ = [("n_reads", ctypes.c_int64), ("bools", ctypes.c_void_p * 9), ("bools_validity", ctypes.c_void_p * 9),
                ("reference_id", ctypes.c_void_p), ("reference_id_validity", ctypes.c_void_p),
                ("mate_reference_id", ctypes.c_void_p), ("mate_reference_id_validity", ctypes.c_void_p),
                ("mapq", ctypes.c_void_p), ("mapq_validity", ctypes.c_void_p)]


_SIG = {
    "bqsr_sam_flagstat": (ctypes.c_int, [vp, vp, vp, ctypes.POINTER(_FlagStat)]),
    "bqsr_flagstat_arrow": (ctypes.c_int, [vp, ctypes.POINTER(FlagStatChunk), i32, vp, ctypes.POINTER(_FlagStat)]),
    "bqsr_flagstat_arrow_device": (ctypes.c_int, [vp, ctypes.POINTER(FlagStatChunk), vp, vp]),
}


def _lib():
    return _capi.bind(_capi.lib(), _SIG)


def _result(r: _FlagStat) -> Tuple[FlagStatMetrics, FlagStatMetrics]:
    """(failed, passed): adamFlagStat's order"""
    return FlagStatMetrics(*list(r.failed.c)), FlagStatMetrics(*list(r.passed.c))


def sam_flagstat(sam, stream=None) -> Tuple[FlagStatMetrics, FlagStatMetrics]:
    """bqsr_sam_flagstat over a sam.SamText: (failed, passed)"""
    r = _FlagStat()
    check(_lib().bqsr_sam_flagstat(sam.ctx.handle, sam.h, stream, ctypes.byref(r)))
    return _result(r)


def arrow_flagstat(chunks, ctx: Optional[bqsr.Context] = None, stream=None
                   ) -> Tuple[FlagStatMetrics, FlagStatMetrics]:
    """bqsr_flagstat_arrow over FlagStatChunk structures (host pointers the
    caller keeps alive): (failed, passed)"""
    ctx = ctx or bqsr.Context.get(0)
    arr = (FlagStatChunk * max(1, len(chunks)))(*chunks)
    r = _FlagStat()
    check(_lib().bqsr_flagstat_arrow(ctx.handle, arr, len(chunks), stream, ctypes.byref(r)))
    return _result(r)


def table_chunks(table):
    """(chunks, keep): one FlagStatChunk per record batch of an Arrow table
    holding (some of) PROJECTION's columns, arrays normalised to offset 0;
    `keep` owns the buffers the chunks point into."""
    import pyarrow as pa
    names = set(table.column_names)
    keep = []

    def flat(a, typ):
        if a.type != typ:
            a = a.cast(typ)
        if a.offset:
            a = pa.concat_arrays([a])
        keep.append(a)
        return a

    def addr(b):
        return None if b is None else b.address

    chunks = []
    for rb in table.to_batches():
        if rb.num_rows == 0:
            continue
        C = FlagStatChunk()
        C.n_reads = rb.num_rows
        for k, name in enumerate(BOOL_COLUMNS):
            if name in names:
                b = flat(rb.column(rb.schema.get_field_index(name)), pa.bool_()).buffers()
                C.bools[k], C.bools_validity[k] = addr(b[1]), addr(b[0])
        for name, attr in zip(INT_COLUMNS, ("reference_id", "mate_reference_id", "mapq")):
            if name in names:
                b = flat(rb.column(rb.schema.get_field_index(name)), pa.int32()).buffers()
                setattr(C, attr, addr(b[1]))
                setattr(C, attr + "_validity", addr(b[0]))
        chunks.append(C)
    return chunks, keep


def _flagstat(path: str, device: int, partition_bytes: int, region=None, bai=None):
    region = region_plan(path, region, bai)  # (refused before anything is read)
    ctx = bqsr.Context.get(device)
    ph = Phases()
    failed, passed = FlagStatMetrics(), FlagStatMetrics()
    stats: Dict[str, object] = {"reads": 0}
    if is_parquet(path):
        from . import parquet as P
        with ph("read"):
            table = P.read_table(path, columns=PROJECTION)
            chunks, keep = table_chunks(table)
        with ph("flagstat"):
            failed, passed = arrow_flagstat(chunks, ctx)
        del keep
        stats["reads"] = table.num_rows
    else:
        with SamInput(path, ctx, ph, partition_bytes, region=region, bai=bai) as src:
            if not src.bam and len(src.data):
                stats["partitions"] = src.n_partitions
            for sam, base in src:
                stats.update(src.region_stats or {})
                with ph("flagstat"):
                    try:
                        f, p = sam_flagstat(sam)
                    except _capi.BQSRError as e:
                        raise rebased(e, base) from None
                failed, passed = failed + f, passed + p
                stats["reads"] = base + sam.counts().n_reads
    stats["phases"] = ph.t
    return failed, passed, stats


def flagstat(path: str, device: int = 0, partition_bytes: Optional[int] = None, region: Optional[str] = None,
             bai: Optional[str] = None) -> Tuple[FlagStatMetrics, FlagStatMetrics]:
    """adamFlagStat of a SAM, BAM or ADAMRecord Parquet input: (failed,
    passed), the reference's order (rdd/FlagStat.scala:102-114).
    partition_bytes: SAM text per streamed partition (default:
    inputs.DEFAULT_PARTITION_BYTES).  region (BAM input): only the reads that
    overlap it, read through the .bai index (inputs.SamInput)."""
    f, p, _ = _flagstat(path, device, DEFAULT_PARTITION_BYTES if partition_bytes is None else partition_bytes, region, bai)
    return f, p


def percent(fraction: int, total: int) -> float:
    """cli/FlagStat.scala:63: 0.0 for an empty total, else the double
    100.0 * fraction.toFloat / total -- the count passes through a 32-bit float."""
    if total == 0:
        return 0.0
    return 100.0 * struct.unpack("f", struct.pack("f", fraction))[0] / total


def java_2f(x: float) -> str:
    """Java's "%.2f" of a double: the shortest decimal that round-trips
    (Double.toString's digits; Python's repr) rounded half up to two places --
    not C's exact-binary-value rounding: 0.125 gives "0.13".  JDKs before 19
    occasionally print a Double.toString that is not the shortest; that is not
    reproduced here."""
    return str(decimal.Decimal(repr(float(x))).quantize(decimal.Decimal("0.01"), rounding=decimal.ROUND_HALF_UP))


_LINES = (("total", "in total (QC-passed reads + QC-failed reads)", False),
          ("dup_primary_total", "primary duplicates", False),
          ("dup_primary_both_mapped", "primary duplicates - both read and mate mapped", False),
          ("dup_primary_only_read_mapped", "primary duplicates - only read mapped", False),
          ("dup_primary_cross_chromosome", "primary duplicates - cross chromosome", False),
          ("dup_secondary_total", "secondary duplicates", False),
          ("dup_secondary_both_mapped", "secondary duplicates - both read and mate mapped", False),
          ("dup_secondary_only_read_mapped", "secondary duplicates - only read mapped", False),
          ("dup_secondary_cross_chromosome", "secondary duplicates - cross chromosome", False),
          ("mapped", "mapped", True),
          ("paired_in_sequencing", "paired in sequencing", False),
          ("read1", "read1", False),
          ("read2", "read2", False),
          ("properly_paired", "properly paired", True),
          ("with_self_and_mate_mapped", "with itself and mate mapped", False),
          ("singleton", "singletons", True),
          ("with_mate_mapped_to_diff_chromosome", "with mate mapped to a different chr", False),
          ("with_mate_mapped_to_diff_chromosome_mapq5", "with mate mapped to a different chr (mapQ>=5)", False))


def format_flagstat(failed: FlagStatMetrics, passed: FlagStatMetrics) -> str:
    """The text cli/FlagStat.scala:65-108 hands to println (print() adds the
    final newline as println does): a line break, eighteen "%d + %d ..." lines
    (passed first), then a line of thirteen spaces.  Percentages as java_2f."""
    out = [""]
    for name, words, pct in _LINES:
        p, f = getattr(passed, name), getattr(failed, name)
        line = "%d + %d %s" % (p, f, words)
        if pct:
            line += " (%s%%:%s%%)" % (java_2f(percent(p, passed.total)), java_2f(percent(f, failed.total)))
        out.append(line)
    out.append(" " * 13)
    return "\n".join(out)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="adam_amd.flagstat", description=__doc__.split("\n\n")[0])
    ap.add_argument("input")
    ap.add_argument("-partition_bytes", type=int, default=DEFAULT_PARTITION_BYTES,
                    help="SAM text per streamed partition, in bytes")
    add_region_arguments(ap)
    a = ap.parse_args(argv)
    try:
        a.region = region_plan(a.input, a.region, a.bai)
    except (ValueError, OSError) as e:
        ap.error(str(e))
    t0 = time.perf_counter()
    failed, passed, st = _flagstat(a.input, 0, a.partition_bytes, a.region, a.bai)
    print(format_flagstat(failed, passed))
    report(st, t0)
    return 0


if __name__ == "__main__":
    sys.exit(main())
