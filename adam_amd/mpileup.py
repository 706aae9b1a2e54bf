"""`adam mpileup` on the device: pileup text by position.

The reference's MpileupCommand (adam-cli/.../cli/MpileupCommand.scala:37-82)
walks a PileupTraversable (adam-core/.../util/PileupTraversable.scala:83-281)
over the reads LocusPredicate keeps and prints one line per reference
position: name, 0-based position, reference base, number of events, then the
events -- ``.`` / ``,`` per match, the read's base per mismatch (lower case on
the reverse strand), ``-1`` + the reference base per deleted base, ``+`` + the
read's length + the read's WHOLE sequence per ``I`` element.  Here the walk,
the grouping by position (a stable radix sort) and the formatting of the text
run on the GPU (include/adam_sam.h ``bqsr_sam_mpileup_*`` /
``bqsr_arrow_mpileup_*``, adam_amd/csrc/mpileup.hip); the text comes back in
windows of whole lines, so device and pinned memory stay bounded.

What is kept from the reference, quirks included:

* LocusPredicate (readMapped, primaryAlignment, !failedVendorQualityChecks,
  !duplicateRead; a null fails).  The reference reads Parquet only; SAM and
  BAM are accepted here as everywhere else and the predicate is applied to
  them as well, on the records SAMRecordConverter would produce -- so a
  FLAG-0 record, whose booleans are all false, is dropped.
* A read without CIGAR or MD gives no events but takes part in the ordering.
  No soft-clip events; one insertion event per ``I`` element; the reference
  base of every event from the MD (of a match: the read's own base); after an
  ``N`` the MD is looked up in the wrong place, as in reads2ref.  ``Base`` is
  the five-value enum A C T G N: anything else in the sequence or the MD
  fails the job, as does a MAPQ of 255 (a null mapq) on a read with events.
* A line whose events are all insertions prints ``?`` for the base.

What this project declares where the reference is loose:

* **Order.**  Within a run of one referenceId (a *segment*; a reference that
  comes back later is a new segment) start must not decrease from one kept
  read to the next.  The reference asserts only against the segment's first
  start and prints some positions twice for other disorder; here any decrease
  fails the job with status UNSORTED naming the read
  (``transform -sort_reads`` sorts).
* **Conflict.**  A position whose events disagree on the reference base fails
  the job with status REFERENCE_CONFLICT naming the reference and the
  position: the reference's AssertionError.
* **Failure.**  On any failure nothing is printed and no output file appears
  (the reference would have printed the lines flushed so far).  A read-level
  exception wins, then the lowest unsorted read, then the lowest conflict.
* One input stays resident per job; one that does not fit the device fails
  with a message naming the limit.

    python -m adam_amd.mpileup INPUT.{sam,bam,adam} [-output FILE] [-window_bytes N]
"""
from __future__ import annotations

import argparse
import ctypes
import os
import sys
import time
from typing import Dict, Iterator, Optional, Sequence

import numpy as np

from . import _capi, bqsr
from ._capi import check, dblp, i32, i64, i64p, vp
from .inputs import Phases, SamInput, add_region_arguments, is_parquet, region_plan, report, text_output

# Text per window.  A window's bytes exist once on the device and once in
# pinned host memory; 64 MiB keeps both small beside either memory and is far
# above what the fixed cost of a call shows in.  A line must fit a window.
DEFAULT_WINDOW_BYTES = 64 << 20

LOCUS_COLUMNS = ("readMapped", "primaryAlignment", "failedVendorQualityChecks", "duplicateRead")
# the ADAMRecord columns mpileup reads from Parquet
PROJECTION = ("referenceName", "referenceId", "start", "mapq", "readName", "sequence", "cigar", "qual",
              "readNegativeStrand", "mismatchingPositions") + LOCUS_COLUMNS
KERNELS = ("walk", "emit", "sort", "group", "text")


class MpileupSizes(ctypes.Structure):
    _fields_ = [("n_reads", ctypes.c_int64), ("n_events", ctypes.c_int64), ("n_lines", ctypes.c_int64),
                ("text_bytes", ctypes.c_int64)]


_SIG = {
    "bqsr_sam_mpileup_prepare": (ctypes.c_int, [vp, vp, vp, ctypes.POINTER(MpileupSizes)]),
    "bqsr_arrow_mpileup_prepare": (ctypes.c_int, [vp, vp, vp, vp, vp, i32, ctypes.POINTER(ctypes.c_char_p), i32, vp,
                                                  ctypes.POINTER(MpileupSizes)]),
    "bqsr_sam_mpileup_text": (ctypes.c_int, [vp, vp, i64, i64, vp, vp, i64p, i64p]),
    "bqsr_arrow_mpileup_text": (ctypes.c_int, [vp, vp, i64, i64, vp, vp, i64p, i64p]),
    "bqsr_mpileup_kernel_times": (ctypes.c_int, [dblp]),
}


def _lib():
    return _capi.bind(_capi.lib(), _SIG)


def kernel_times() -> Dict[str, float]:
    """ms by device events of this thread's last prepare (walk, emit, sort,
    group) and last text call (text) (measurement only)"""
    return _capi.stage_times(_lib().bqsr_mpileup_kernel_times, KERNELS, array=True)


def _windows(text_call, handle, ctx, sizes: MpileupSizes, window_bytes: int, stream=None) -> Iterator[bytes]:
    from .adam_save import _pinned
    window_bytes = int(window_bytes)
    if window_bytes < 1:
        raise ValueError("window_bytes must be at least 1")
    line = 0
    buf = None
    nl, nb = ctypes.c_int64(), ctypes.c_int64()
    while line < sizes.n_lines:
        if buf is None:
            buf = _pinned(min(window_bytes, sizes.text_bytes))
        check(text_call(ctx.handle, handle, line, min(window_bytes, sizes.text_bytes), buf.ctypes.data, stream,
                        ctypes.byref(nl), ctypes.byref(nb)))
        line += nl.value
        yield buf[:nb.value].tobytes()


def sam_prepare(sam, stream=None) -> MpileupSizes:
    """bqsr_sam_mpileup_prepare over a sam.SamText: the job's sizes"""
    sz = MpileupSizes()
    check(_lib().bqsr_sam_mpileup_prepare(sam.ctx.handle, sam.h, stream, ctypes.byref(sz)))
    return sz


def sam_mpileup(sam, window_bytes: int = DEFAULT_WINDOW_BYTES, stream=None, sizes: Optional[MpileupSizes] = None):
    """The pileup text of a sam.SamText's reads, as an iterator over windows
    of whole lines (bytes), at most window_bytes each.  The job is prepared
    -- and every read-level, order or conflict failure raised -- before the
    first window is produced."""
    sz = sizes or sam_prepare(sam, stream)
    return _windows(_lib().bqsr_sam_mpileup_text, sam.h, sam.ctx, sz, window_bytes, stream)


def arrow_prepare(reads, stream=None) -> MpileupSizes:
    """bqsr_arrow_mpileup_prepare over a parquet.ArrowReads loaded with
    markdup=True (readName and referenceId travel with MarkDuplicates'
    columns)"""
    import pyarrow as pa
    L = _lib()
    if not getattr(reads, "markdup", False):
        raise ValueError("mpileup needs an ArrowReads loaded with markdup=True (readName and referenceId)")
    table = reads.table
    keep, lens, vals, valids = [], [], [], []
    if not getattr(reads, "_mapq_sent", False) and "mapq" in table.column_names:
        for rb in table.to_batches():
            if rb.num_rows == 0:
                continue
            c = rb.column(rb.schema.get_field_index("mapq"))
            c = c if c.type == pa.int32() else c.cast(pa.int32())
            if c.offset:
                c = pa.concat_arrays([c])
            keep.append(c)
            b = c.buffers()
            lens.append(rb.num_rows)
            vals.append(b[1].address)
            valids.append(b[0].address if b[0] is not None else None)
    k = len(lens)
    names = [s.encode() for s in reads.ref_names]
    a_names = (ctypes.c_char_p * max(1, len(names)))(*names)
    sz = MpileupSizes()
    check(L.bqsr_arrow_mpileup_prepare(reads.ctx.handle, reads.h, (ctypes.c_int64 * max(1, k))(*lens),
                                       (ctypes.c_void_p * max(1, k))(*vals), (ctypes.c_void_p * max(1, k))(*valids), k,
                                       a_names, len(names), stream, ctypes.byref(sz)))
    del keep
    if k:
        reads._mapq_sent = True
    return sz


def arrow_mpileup(reads, window_bytes: int = DEFAULT_WINDOW_BYTES, stream=None, sizes: Optional[MpileupSizes] = None):
    """As :func:`sam_mpileup` over a parquet.ArrowReads (its table as given:
    apply reads2ref.locus_filter before the upload -- the handle carries no
    failedVendorQualityChecks)."""
    sz = sizes or arrow_prepare(reads, stream)
    return _windows(_lib().bqsr_arrow_mpileup_text, reads.h, reads.ctx, sz, window_bytes, stream)


def _filtered(table):
    """(the rows LocusPredicate keeps, their indices in `table`)"""
    import pyarrow as pa
    from .reads2ref import locus_filter
    col = "__mpileup_row"
    kept = locus_filter(table.append_column(col, pa.array(np.arange(table.num_rows, dtype=np.int64))))
    rows = np.asarray(kept.column(col).to_numpy(), np.int64) if kept.num_rows else np.zeros(0, np.int64)
    return kept.drop_columns([col]), rows


def _input_row(e: _capi.BQSRError, rows) -> _capi.BQSRError:
    """the error naming the read by its index in the table :func:`_filtered`
    was given, not among the rows it kept"""
    if e.status == _capi.REFERENCE_CONFLICT or e.read < 0:
        return e
    row = int(rows[e.read])
    msg = str(e).split(": ", 1)[1].replace("read %d" % e.read, "read %d" % row, 1)
    return _capi.BQSRError(e.status, msg, row)


def mpileup(inp: str, out: Optional[str] = None, window_bytes: int = DEFAULT_WINDOW_BYTES, device: int = 0,
            stdout=None, region: Optional[str] = None, bai: Optional[str] = None) -> Dict[str, object]:
    """`adam mpileup`: the pileup text of a SAM, BAM or ADAMRecord Parquet
    input, to `out` or, without it, to stdout (inputs.text_output: the job's
    checks have passed before the first byte is written).  Returns the job's
    statistics; raises :class:`_capi.BQSRError` as the module doc says
    (``.read``: the read's index in the input; for REFERENCE_CONFLICT the
    position).  region, bai: BAM input read through its .bai index, only the reads that overlap the region (inputs.SamInput)."""
    if int(window_bytes) < 1:
        raise ValueError("window_bytes must be at least 1")
    region = region_plan(inp, region, bai)  # (refused before anything is read or created)
    ph = Phases()
    stats: Dict[str, object] = {}
    with text_output(out, stdout) as sink:
        ctx = bqsr.Context.get(device)

        def run(prepare, windows, n_reads):
            with ph("prepare"):
                sz = prepare()
            kt = kernel_times()
            stats.update(reads=n_reads, kept=sz.n_reads, events=sz.n_events, lines=sz.n_lines, bytes=sz.text_bytes)
            text_ms = 0.0
            it = windows(sz)
            while True:
                with ph("text"):
                    w = next(it, None)
                if w is None:
                    break
                text_ms += kernel_times()["text"]
                with ph("write"):
                    sink.write(w)
            kt["text"] = text_ms
            stats["kernel_ms"] = kt

        if is_parquet(inp):
            from . import parquet as P
            with ph("read"):
                table, rows = _filtered(P.read_table(inp, columns=PROJECTION))
            with ph("parse"):
                A = P.ArrowReads(table, ctx, markdup=True)
            try:
                try:
                    run(lambda: arrow_prepare(A), lambda sz: arrow_mpileup(A, window_bytes, sizes=sz), len(rows))
                except _capi.BQSRError as e:
                    raise _input_row(e, rows) from None
            finally:
                A.close()
        else:
            with SamInput(inp, ctx, ph, region=region, bai=bai) as src:
                for sam, _ in src:
                    stats.update(src.region_stats or {})
                    run(lambda: sam_prepare(sam), lambda sz: sam_mpileup(sam, window_bytes, sizes=sz),
                        sam.counts().n_reads)
    stats["phases"] = ph.t
    return stats


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="adam_amd.mpileup", description=__doc__.split("\n\n")[0])
    ap.add_argument("input")
    ap.add_argument("-output", default=None, help="write the text here (default: stdout)")
    ap.add_argument("-window_bytes", type=int, default=DEFAULT_WINDOW_BYTES,
                    help="text per window, in bytes; a line must fit")
    add_region_arguments(ap)
    a = ap.parse_args(argv)
    if a.window_bytes < 1:
        ap.error("-window_bytes must be at least 1")
    if not os.path.exists(a.input):
        ap.error("no such input: %s" % a.input)
    try:
        a.region = region_plan(a.input, a.region, a.bai)
    except (ValueError, OSError) as e:
        ap.error(str(e))
    t0 = time.perf_counter()
    st = mpileup(a.input, a.output, a.window_bytes, region=a.region, bai=a.bai)
    report(st, t0)
    return 0


if __name__ == "__main__":
    sys.exit(main())
