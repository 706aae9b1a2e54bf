"""`adam transform`: the CLI harness around the device path
(adam-cli/.../cli/Transform.scala:38-110).

    python -m adam_amd.transform INPUT.sam OUTPUT.sam [-mark_duplicate_reads]
        [-recalibrate_base_qualities] [-dbsnp_sites SITES.vcf]
    python -m adam_amd.transform INPUT.{adam,parquet,sam} OUTPUT.{adam,parquet} [...]
    python -m adam_amd.transform INPUT.{sam,bam} OUTPUT.{adam,parquet} -parquet_encoder device [...]
    python -m adam_amd.transform INPUT.{sam,bam} OUTPUT.bam [-bam_compression_level N]
        [-bam_compressor {host,device}] [-bam_index] [...]
    python -m adam_amd.transform INPUT.{sam,bam} OUTPUT.adam -parquet_encoder device -parquet_compression snappy
        -parquet_compressor device [...]

SAM or BAM in goes through the device path described below, out as SAM text,
as BAM (an output name ending in .bam: the records encoded on the device,
sam.SamText.bam_records, cut into BGZF members compressed by host threads,
sam.bgzf_compress, or with -bam_compressor device deflated on the device,
sam.SamText.bam_members; see _BamOut) or as ADAMRecord Parquet part files (adamSave,
adam_save.py).  BAM holds what the SAM spec allows: a record it cannot hold
-- the reference's trimmed recalibrated QUAL strings and its chars above
0x7F among them, which the SAM text sink writes as they are -- fails the job
with BQSRError (UNSUPPORTED) naming the read, and no output appears.
ADAMRecord Parquet input cannot be written as BAM here (that path has no SAM
lines to encode): a ValueError before anything is read; `adam2sam`
(adam2sam.py) renders the lines and writes SAM or BAM.  ADAMRecord
Parquet in goes through ``transform_parquet``: Arrow decodes the Parquet
pages on host threads, the column buffers go to the device as they are
(parquet.ArrowReads), MarkDuplicates, the BQSR batch and the recalibrated
qual column are built there, and the records are written back as Parquet
with the qual (and duplicateRead) columns replaced.

Steps in Transform.run's order (:66-90): load (the SAM text parsed on the
device, SAMRecordConverter semantics), MarkDuplicates (`adamMarkDuplicates`),
BQSR (`adamBQSR(loadSnpTable)`: an empty SnpTable without -dbsnp_sites,
:96-105), save.  The output is ADAMRecord Parquet part files, as the
reference's adamSave writes them (core/rdd/AdamRDDFunctions.scala:37-56;
OUTPUT.adam / .parquet / a directory), or SAM text -- the input records with
their QUAL fields replaced by the recalibrated strings (and FLAG 0x400 by
MarkDuplicates' result).  -coalesce and -realignIndels are outside this
build and are refused.

-parquet_encoder device (SAM or BAM in, ADAM out; gzip, snappy or none): the
part files' data pages are encoded on the device from the columns the ADAM
passes leave there (adam_pages.py, parquet_pages.py), and only the encoded
pages come down; the default, host, copies the columns down and has pyarrow
encode them.  Both write the same records; the device encoder writes cigar
PLAIN, the host encoder through a dictionary.  Refused before anything is
read: SAM or BAM output, ADAM Parquet input (transform_parquet keeps its
writer), zstd.  -parquet_compressor device (only with -parquet_encoder device
-parquet_compression snappy; refused otherwise before anything is read or
created) compresses those data pages on the device too
(adam_amd/csrc/snappy_pages.hip) and only the compressed pages come down.

-sort_reads (adamSortReadsByReferencePosition,
core/rdd/AdamRDDFunctions.scala:63-93; the last step before the save,
cli/Transform.scala:89-93) sorts the records on the device (sam.SamText.sort:
mapped reads by (referenceId, start), then the unmapped ones in the
reference's counter order, ties in input order): the recalibrated text is
written on the device, its records are sorted there and the sinks read the
sorted parse.  ADAM Parquet input is sorted by `table.take` of the order the
device computes from the readMapped / referenceId / start columns
(sam.sort_order).  The input must be one partition: a global sort across
streamed partitions is not built, and an input cut into several raises a
ValueError before anything is read.

Partitions: an input whose records exceed ``partition_bytes`` is cut at line
boundaries into partitions (the Hadoop splits the reference's RDD is read
as, each parsed with the header as a SAM file of its own) that stream through
the device: every partition is parsed and packed into a resident batch and
observed into the one count table (computeTable's per-partition aggregate
merged by ``RecalTable.++``, RecalibrateBaseQualities.scala:52-64), the
per-partition expectedMismatch values folded in partition order, then per
partition: apply, its text re-read (the reference re-reads its input per
stage, cli/Transform.scala:62-97), QUAL rewritten on the device and the
records appended to the output.  Errors are raised in the reference's order:
observe errors partition by partition, finalize, then apply errors partition
by partition; the output file appears only when the job succeeds.
MarkDuplicates groups reads across the whole input (its groupBy): with
-mark_duplicate_reads every partition is parsed once more up front and its
reads' compact MarkDuplicates records (sam.DupSet, bqsr_dup_set_*) collected
on the device; the duplicate bits, found over all partitions, are set on each
partition's parse before BQSR observes it and before it is written.
"""
from __future__ import annotations

import argparse
import ctypes
import os
import shutil
import sys
import time
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _capi, bqsr
from . import distributed as D
from ._capi import check
from .adam_save import check_out as _check_out
from .inputs import DEFAULT_PARTITION_BYTES, SamInput, add_region_arguments, is_bam, is_parquet, region_plan, report, sam_partitions  # noqa: F401
from .inputs import Phases as _Phases, host_bytes as _host_bytes  # noqa: F401
from .parquet_pages import COMPRESSORS as PARQUET_COMPRESSORS, compressor_refusal
from .sam import SamText

def _bqsr_partitions(data, header: bytes, ranges: List[Tuple[int, int]], snp, ctx, device: int, emit,
                     max_exc: int = 1 << 16, dups=None) -> Dict[str, float]:
    """BQSR over several partitions of one SAM input (see the module doc);
    emit(i, sam) gets every partition's parse with its QUAL fields rewritten,
    in partition order (emit(i, sam, quals): quals = the apply's outputs for
    the parse, handed to the sink).  dups: a finished sam.DupSet over the same
    partitions (MarkDuplicates' bits set on every parse before its batch is
    built and before it is rewritten)."""
    import torch
    L = _capi.lib()
    dev = torch.device("cuda", device)
    stream = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    h = ctx.handle
    contigs = snp.contigs if snp else None
    sites_h = snp.handle(ctx) if snp else None
    batches: List[ctypes.c_void_p] = []
    th, lut = ctypes.c_void_p(), ctypes.c_void_p()
    n_reads = 0
    try:
        # (1) every partition parsed on the device and packed into a resident batch
        n_rg = max_len = 1
        slots, reads = [], []
        for a, b in ranges:
            sam = SamText(header + bytes(data[a:b]), ctx)
            try:
                if dups is not None:
                    dups.apply(len(batches), sam)
                bh = sam.device_batch(contigs, sp)  # packed on the device
            finally:
                sam.close()
            batches.append(bh)
            d = L.bqsr_batch_dims(bh)
            n_rg, max_len = max(n_rg, d.n_rg), max(max_len, d.max_len)
            slots.append(int(L.bqsr_batch_slots(bh)))
            reads.append(int(L.bqsr_batch_reads(bh)))
        n_reads = sum(reads)
        # (2) computeTable: every partition observed into the one table, its
        # errors raised partition by partition, expectedMismatch folded in
        # partition order
        dims = _capi.Dims(n_rg, max_len)
        table = torch.zeros(int(L.bqsr_table_words(dims)), dtype=torch.int64, device=dev)
        check(L.bqsr_table_create(h, dims, ctypes.c_void_p(table.data_ptr()), ctypes.byref(th)))
        em = torch.zeros(max(1, len(batches)), dtype=torch.float64, device=dev)
        for i, bh in enumerate(batches):
            check(L.bqsr_observe_async(h, bh, sites_h, th, sp))
            check(L.bqsr_batch_em_copy_async(bh, ctypes.c_void_p(em.data_ptr() + 8 * i), sp))
        for bh in batches:
            v = ctypes.c_double()
            check(L.bqsr_observe_result(bh, ctypes.byref(v), sp))
        acc = D.fold_partition_ems_device(em[:len(batches)], [len(batches)], ctx, stream)
        check(L.bqsr_finalize_device(h, th, ctypes.c_void_p(acc.data_ptr()), ctypes.byref(lut), sp))
        # (3) applyTable partition by partition, each partition's records
        # re-read, rewritten on the device and appended
        out_qual = torch.empty(max(slots or [0]) + 64, dtype=torch.uint8, device=dev)
        out_start = torch.empty(max(1, max(reads or [1])), dtype=torch.int32, device=dev)
        out_len = torch.empty_like(out_start)
        exc = torch.empty(max_exc, dtype=torch.int64, device=dev)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        for i, (a, b) in enumerate(ranges):
            bh = batches[i]
            check(L.bqsr_apply_stage(h, bh, lut, ptr(out_qual), ptr(out_start), ptr(out_len), ptr(exc), max_exc,
                                     _capi.STAGE_RESET | _capi.STAGE_KERNEL, sp))
            v, nexc = ctypes.c_double(), ctypes.c_int64()
            check(L.bqsr_job_result(bh, lut, ctypes.byref(v), ctypes.byref(nexc), sp))
            if nexc.value > max_exc:
                raise _capi.BQSRError(_capi.UNSUPPORTED, "partition %d: %d chars above 0xFF exceed the exception "
                                      "list" % (i, nexc.value))
            sam = SamText(header + bytes(data[a:b]), ctx)
            try:
                if dups is not None:
                    dups.apply(i, sam)
                emit(i, sam, (bh, ptr(out_qual), ptr(out_start), ptr(out_len), ptr(exc), nexc.value, sp))
            finally:
                sam.close()
            L.bqsr_batch_destroy(bh)
            batches[i] = None
    finally:
        if lut:
            L.bqsr_lut_destroy(lut)
        if th:
            L.bqsr_table_destroy(th)
        for bh in batches:
            if bh:
                L.bqsr_batch_destroy(bh)
    return {"reads": n_reads, "partitions": len(ranges)}


def _partitions(data, header: bytes, ranges, mark_duplicates: bool, recalibrate: bool, dbsnp, ctx, device: int,
                emit) -> Dict[str, float]:
    """A SAM input of several partitions: MarkDuplicates over all of them
    (a DupSet: every partition parsed once for its compact records), then
    BQSR over the partitions streamed through the device, or (without BQSR)
    every partition re-parsed, its FLAG fields rewritten and emitted."""
    from .sam import DupSet
    dups = None
    stats: Dict[str, float] = {}
    try:
        if mark_duplicates:
            dups = DupSet(ctx)
            for a, b in ranges:
                sam = SamText(header + bytes(data[a:b]), ctx)
                try:
                    dups.add(sam)
                finally:
                    sam.close()
            n_dup = dups.finish()
        if recalibrate:
            snp = bqsr.SnpTable.from_vcf(dbsnp) if dbsnp else bqsr.SnpTable()
            stats = _bqsr_partitions(data, header, ranges, snp if snp.table else None, ctx, device, emit,
                                     dups=dups)
        else:
            n_reads = 0
            for i, (a, b) in enumerate(ranges):
                sam = SamText(header + bytes(data[a:b]), ctx)
                try:
                    n_reads += sam.counts().n_reads
                    dups.apply(i, sam)
                    emit(i, sam, None)
                finally:
                    sam.close()
            stats = {"reads": n_reads, "partitions": len(ranges)}
        if dups is not None:
            stats["duplicates"] = n_dup
    finally:
        if dups is not None:
            dups.close()
    return stats


def transform_parquet(inp: str, out: str, mark_duplicates: bool = False, recalibrate: bool = False,
                      dbsnp: Optional[str] = None, device: int = 0, overwrite: bool = False,
                      sort_reads: bool = False) -> Dict[str, float]:
    """`transform` with ADAMRecord Parquet output (adamSave,
    core/rdd/AdamRDDFunctions.scala:37-56): the input -- Parquet (adamLoad,
    AdamContext.scala:318-331, every column kept and written back) or SAM
    (parsed on the host); for Parquet input the Arrow columns go to the device
    (parquet.ArrowReads): MarkDuplicates, the BQSR batch and the rebuilt qual
    column all built there; the qual (and duplicateRead) columns replaced."""
    from . import parquet as P
    from .records import RecordBatch, read_sam_records
    _check_out(out, overwrite, True)
    t0 = time.perf_counter()
    batch = None
    A = None
    if is_parquet(inp):
        table = P.read_table(inp)
    else:
        if mark_duplicates:  # (the host SAM parse carries no library / mateMapped: use SAM output or ADAM input)
            raise ValueError("-mark_duplicate_reads with SAM input and ADAM output is not supported")
        recs = read_sam_records(inp)
        batch = RecordBatch.from_records(recs)
        table = P.batch_to_table(batch, [r.read_name for r in recs])
    n = table.num_rows
    stats: Dict[str, float] = {"reads": n}
    if is_parquet(inp) and (mark_duplicates or recalibrate):
        # the Arrow columns on the device: MarkDuplicates there, the batch
        # packed there, the qual column rebuilt there after apply
        cols = [c for c in table.column_names if c in P.BQSR_PROJECTION or c in P.MARKDUP_PROJECTION]
        A = P.ArrowReads(table.select(cols), bqsr.Context.get(device), markdup=mark_duplicates)
    try:
        return _transform_table(A, table, batch, inp, out, mark_duplicates, recalibrate, dbsnp, device, stats, t0,
                                sort_reads)
    finally:
        if A is not None:
            A.close()


def table_sort_order(table, ctx=None) -> np.ndarray:
    """-sort_reads over an ADAMRecord table: the order sam.sort_order gives
    its readMapped (null: false), referenceId and start columns"""
    from .records import F_HAS_START, F_MAPPED
    from .sam import sort_order
    n = table.num_rows

    def col(name, dtype, null):
        if name not in table.column_names:
            return np.full(n, null, dtype), np.zeros(n, bool)
        c = table.column(name).combine_chunks()
        valid = np.asarray(c.is_valid())
        return np.asarray(c.fill_null(null)).astype(dtype), valid
    mapped, _ = col("readMapped", bool, False)
    ref, ref_ok = col("referenceId", np.int64, 0)
    start, start_ok = col("start", np.int64, 0)
    if np.any(mapped & ref_ok & ((ref < 0) | (ref > 0x7FFFFFFF))):
        raise _capi.BQSRError(_capi.UNSUPPORTED, "sort_reads: a referenceId outside [0, Int.MaxValue]")
    flags = np.where(mapped, np.uint32(F_MAPPED), np.uint32(0)) | np.where(start_ok, np.uint32(F_HAS_START),
                                                                            np.uint32(0))
    return sort_order(flags.astype(np.uint32), np.where(ref_ok, ref, -1).astype(np.int32), start, ctx)


def _transform_table(A, table, batch, inp, out, mark_duplicates, recalibrate, dbsnp, device, stats, t0,
                     sort_reads=False):
    import pyarrow.parquet as pq

    from . import parquet as P
    from .records import F_DUPLICATE
    n = table.num_rows
    if mark_duplicates:
        stats["duplicates"] = A.mark_duplicates()
        dcol = A.flag_column(F_DUPLICATE)
        table = (table.set_column(table.column_names.index("duplicateRead"), "duplicateRead", dcol)
                 if "duplicateRead" in table.column_names else table.append_column("duplicateRead", dcol))
    if recalibrate:
        snp = bqsr.SnpTable.from_vcf(dbsnp) if dbsnp else bqsr.SnpTable()
        if A is not None:
            from .job import ResidentJob
            job = ResidentJob(None, None, snp if snp.table else None, device,
                              handle=A.device_batch(snp.contigs if snp.table else None))
            try:
                job.step()
                qcol = A.qual_column(job)
            finally:
                job.close()
        else:
            parts = bqsr.adam_bqsr([batch], snp if snp.table else None, bqsr.Context.get(device))
            qcol = P.recalibrated_qual_column(parts, n)
        table = (table.set_column(table.column_names.index("qual"), "qual", qcol)
                 if "qual" in table.column_names else table.append_column("qual", qcol))
    # the new file first, then the old output goes (a failed write leaves the
    # previous output in place); a leftover part-file directory at the
    # .partial path (_check_out allowed it under overwrite) is removed first
    if sort_reads:  # the last step before the save (cli/Transform.scala:89-93)
        import pyarrow as pa
        table = table.take(pa.array(table_sort_order(table, bqsr.Context.get(device)), pa.int64()))
    tmp = out + ".partial"
    if os.path.isdir(tmp):
        shutil.rmtree(tmp)
    pq.write_table(table, tmp)
    if os.path.isdir(out):  # (transform_parquet checked it: overwrite of a part-file directory)
        shutil.rmtree(out)
    os.replace(tmp, out)
    stats["seconds"] = time.perf_counter() - t0
    return stats


class _SamOut:
    """SAM text output (records appended partition by partition; the file
    appears when the job succeeds)."""

    def __init__(self, path: str, overwrite: bool = False):
        _check_out(path, overwrite, False)
        self.path = path
        self.tmp = path + ".partial"
        self.fh = open(self.tmp, "wb")
        self.first = True

    def emit(self, i, sam, quals=None):
        """quals: (batch, out_qual, out_start, out_len, exceptions, n, stream)
        of an apply over the parse (None: QUAL kept; FLAG after MarkDuplicates)"""
        if quals is None:
            sam.rewrite(None)
        else:
            check(_capi.lib().bqsr_sam_rewrite_quals(sam.ctx.handle, sam.h, *quals))
        text = sam.text()
        self.fh.write(text if self.first else text[self._header_len(sam):])
        self.first = False

    @staticmethod
    def _header_len(sam) -> int:
        from .adam_save import _lib
        n = ctypes.c_int64()
        check(_lib().bqsr_sam_header_text(sam.h, None, 0, ctypes.byref(n)))
        return int(n.value)

    def close(self, ok: bool = True):
        self.fh.close()
        if ok:
            os.replace(self.tmp, self.path)
        elif os.path.exists(self.tmp):
            os.remove(self.tmp)


# Records per encoded piece of BAM output.  A record of a 100-150 base read is
# 250-350 bytes of BAM, so 2^19 records are 130-180 MB: on the device next to
# the text they are encoded from, in host memory as the downloaded stream,
# and once more as BGZF members while the next piece is encoded and downloaded
# -- a few hundred MB in flight whatever the partition's size, small beside HBM
# and host memory; large enough (2000+ members) that the 16 compressing
# threads stay busy and a piece's fixed costs (two launches, a scan, three
# copies) do not show; far below the 2^31 bytes one piece may hold.
BAM_PIECE_READS = 1 << 19


BAM_COMPRESSORS = ("host", "device")
DEVICE_LEVEL_REFUSAL = ("-bam_compressor device has one level: it cannot be combined with an explicit "
                        "-bam_compression_level")


BAM_INDEX_KERNELS = ("rows", "locate", "windows", "sort", "chunks", "serialize_host")
BAM_INDEX_REFUSAL = "-bam_index applies to BAM output only (an output name ending in .bam)"


class BamIndexSizes(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in ("n_records", "n_chunks", "n_bins", "n_windows", "bytes",
                                              "device_bytes")]


_INDEX_SIG = {
    "bqsr_bam_index_create": (ctypes.c_int, [_capi.vp, _capi.i32, _capi.pp]),
    "bqsr_bam_index_destroy": (None, [_capi.vp]),
    "bqsr_bam_index_add": (ctypes.c_int, [_capi.vp, _capi.vp, _capi.i64, _capi.vp]),
    "bqsr_bam_index_set_members": (ctypes.c_int, [_capi.vp, _capi.vp, _capi.i64, _capi.vp]),
    "bqsr_bam_index_finish": (ctypes.c_int, [_capi.vp, _capi.vp]),
    "bqsr_bam_index_size": (ctypes.c_int, [_capi.vp, ctypes.POINTER(BamIndexSizes)]),
    "bqsr_bam_index_bytes": (ctypes.c_int, [_capi.vp, _capi.vp, _capi.i64]),
    "bqsr_bam_index_kernel_times": (ctypes.c_int, [_capi.vp, _capi.dblp]),
}


def _index_lib():
    return _capi.bind(_capi.lib(), _INDEX_SIG)


def bgzf_member_table(data, stream_pos: int, file_pos: int, table: List[int]) -> Tuple[int, int]:
    """The BGZF members of `data` (whole members, as the BAM sink writes
    them) appended to `table` as (stream start, file offset) pairs, walking
    their BSIZE fields; ISIZE advances the stream.  Returns the stream and
    file positions after them."""
    import struct
    p, n = 0, len(data)
    while p < n:
        size = struct.unpack_from("<H", data, p + 16)[0] + 1 if p + 18 <= n else n + 1
        if p + size > n:
            raise ValueError("BAM index: the bytes written do not end on a BGZF member")
        table += (stream_pos, file_pos + p)
        stream_pos += struct.unpack_from("<I", data, p + size - 4)[0]
        p += size
    return stream_pos, file_pos + n


class _BamOut:
    """BAM output with _SamOut's contract (records appended partition by
    partition; the file appears when the job succeeds): the header once,
    then per emit the records in pieces of `piece_reads`, each encoded on the
    device (SamText.bam_records) and compressed into BGZF members by host
    threads (sam.bgzf_compress, `level`: None is 6) while the next piece is
    encoded and downloaded; the EOF marker at close(ok=True).  A piece ends in
    a short member.  compressor="device": each piece's members come deflated
    from the device (SamText.bam_members: the record stream is not downloaded)
    and are written as they arrive, no compressor thread; the header member
    stays on the host path; the device form has one level, so `level` must be
    None.

    index: OUT.bam.bai is written beside the BAM (SAM spec §5.2; the rules are
    in include/adam_sam.h at bqsr_bam_index_create).  Every piece's records
    leave a row each on the device after its prepare (bqsr_bam_index_add);
    the members of every byte written are walked here into the table of
    (stream start, file offset); at close(ok=True) the table goes up, the
    device builds the index (bqsr_bam_index_finish), the host serialises it.
    An output that is not in coordinate order, or a record that ends above
    2^29, raises BQSRError naming the read, and neither file appears.  The
    index goes to OUT.bam.bai.partial and is renamed after the BAM.  Without
    `index` nothing of this is launched or allocated."""

    def __init__(self, path: str, level: Optional[int] = None, piece_reads: int = BAM_PIECE_READS,
                 overwrite: bool = False, compressor: str = "host", index: bool = False):
        from concurrent.futures import ThreadPoolExecutor
        if compressor not in BAM_COMPRESSORS:
            raise ValueError("-bam_compressor must be one of %s" % ", ".join(BAM_COMPRESSORS))
        if compressor == "device" and level is not None:
            raise ValueError(DEVICE_LEVEL_REFUSAL)
        level = 6 if level is None else level
        if not 0 <= int(level) <= 9:
            raise ValueError("-bam_compression_level must be 0..9")
        _check_out(path, overwrite, False)
        if index:
            _check_out(path + ".bai", overwrite, False)
        self.path = path
        self.tmp = path + ".partial"
        self.index = bool(index)
        self.idx = None            # the device index (made at the first emit: it needs the header's n_ref)
        self.members: List[int] = []  # (stream start, file offset) of every member written
        self.stream_pos = 0        # of the record stream: where the next member's bytes start
        self.record_pos = 0        # of the record stream: where the next piece's records start
        self.level = int(level)
        self.compressor = compressor
        self.piece_reads = max(1, int(piece_reads))
        self.fh = open(self.tmp, "wb")
        self.first = True
        self.pool = ThreadPoolExecutor(1)  # (the header member, and the host compressor's pieces)
        self.pending = None
        # measured: the two kernels' device-event ms, stream / file bytes, seconds inside the compressor
        # (device: inside bam_members, pass 2 and the download included), the deflate kernels' ms, bytes downloaded
        self.stats = {"len_ms": 0.0, "write_ms": 0.0, "record_bytes": 0, "text_bytes": 0, "file_bytes": 0,
                      "compress_s": 0.0, "compressor": compressor, "deflate_ms": 0.0, "pack_ms": 0.0,
                      "downloaded_bytes": 0}
        if index:  # the host's member walk, the .bai file's bytes (the stage times arrive at close)
            self.stats.update(index_walk_s=0.0, index_bytes=0)

    def _compress(self, data):
        from .sam import bgzf_compress
        t0 = time.perf_counter()
        out = bgzf_compress(data, self.level)
        self.stats["compress_s"] += time.perf_counter() - t0
        return out

    def _write(self, out):
        self.fh.write(out)
        if self.index:
            t0 = time.perf_counter()
            self.stream_pos, _ = bgzf_member_table(out, self.stream_pos, self.stats["file_bytes"], self.members)
            self.stats["index_walk_s"] += time.perf_counter() - t0
        self.stats["file_bytes"] += len(out)

    def _drain(self):
        if self.pending is not None:
            f, self.pending = self.pending, None
            self._write(f.result())

    def _index_add(self, sam, stream_bytes: int):
        """after the piece's prepare: its records' rows appended on the device"""
        if self.index:
            check(_index_lib().bqsr_bam_index_add(self.idx, sam.h, self.record_pos, None))
            self.record_pos += int(stream_bytes)

    def _index_finish(self) -> bytes:
        """the member table up, the index built on the device, its bytes"""
        L = _index_lib()
        if self.idx is None:  # no emit: a BAM of the EOF marker alone has no references
            return b"BAI\1" + bytes(12)
        table = np.array(self.members + [self.stream_pos, self.stats["file_bytes"]], np.uint64)
        check(L.bqsr_bam_index_set_members(self.idx, table.ctypes.data, len(self.members) // 2, None))
        check(L.bqsr_bam_index_finish(self.idx, None))
        sz = BamIndexSizes()
        check(L.bqsr_bam_index_size(self.idx, ctypes.byref(sz)))
        buf = np.empty(max(1, sz.bytes), np.uint8)
        check(L.bqsr_bam_index_bytes(self.idx, buf.ctypes.data, sz.bytes))
        self.stats["index_bytes"] = int(sz.bytes)
        self.stats["index_chunks"] = int(sz.n_chunks)
        self.stats["index_bins"] = int(sz.n_bins)
        self.stats["index_device_bytes"] = int(sz.device_bytes)
        self.stats["index_ms"] = _capi.stage_times(L.bqsr_bam_index_kernel_times, BAM_INDEX_KERNELS, self.idx,
                                                   array=True)
        return buf[:sz.bytes].tobytes()

    def _submit(self, data):
        self._drain()  # one piece compressing while the next is encoded
        self.pending = self.pool.submit(self._compress, data)

    def emit(self, i, sam, quals=None):
        """as _SamOut.emit: the text rewritten (QUAL from the apply, FLAG
        after MarkDuplicates), then its records encoded and appended"""
        from .sam import bam_kernel_times
        if quals is None:
            sam.rewrite(None)
        else:
            check(_capi.lib().bqsr_sam_rewrite_quals(sam.ctx.handle, sam.h, *quals))
        if self.first:
            head = sam.bam_header()
            if self.index:
                import struct
                self.idx = ctypes.c_void_p()
                n_ref = struct.unpack_from("<i", head, 8 + struct.unpack_from("<i", head, 4)[0])[0]
                check(_index_lib().bqsr_bam_index_create(sam.ctx.handle, n_ref, ctypes.byref(self.idx)))
                self.record_pos = len(head)
            self._submit(head)
            self.first = False
        c = sam.counts()
        self.stats["text_bytes"] += c.text_bytes
        for r0 in range(0, c.n_reads, self.piece_reads):
            n = min(self.piece_reads, c.n_reads - r0)
            if self.compressor == "device":
                self._emit_device(sam, r0, n)
                continue
            rec = sam.bam_records(r0, n)
            self._index_add(sam, rec.size)
            a, b = bam_kernel_times()
            self.stats["len_ms"] += a
            self.stats["write_ms"] += b
            self.stats["record_bytes"] += int(rec.size)
            self.stats["downloaded_bytes"] += int(rec.size)
            self._submit(rec)

    def _emit_device(self, sam, r0: int, n: int):
        """a piece deflated on the device (SamText.bam_members) and written as it arrives"""
        from .sam import BamSizes, bam_kernel_times, bgzf_deflate_times
        sz = BamSizes()
        check(sam.L.bqsr_sam_bam_prepare(sam.ctx.handle, sam.h, int(r0), int(n), None, ctypes.byref(sz)))
        self._index_add(sam, sz.bytes)
        t0 = time.perf_counter()
        out = sam._members(sz.bytes)
        self.stats["compress_s"] += time.perf_counter() - t0
        a, b = bam_kernel_times()
        d, p = bgzf_deflate_times()
        self.stats["len_ms"] += a
        self.stats["write_ms"] += b
        self.stats["deflate_ms"] += d
        self.stats["pack_ms"] += p
        self.stats["record_bytes"] += int(sz.bytes)
        self.stats["downloaded_bytes"] += len(out)
        self._drain()  # (the header member goes first)
        self._write(out)

    def close(self, ok: bool = True):
        from .sam import BGZF_EOF
        bai_tmp = self.path + ".bai.partial"
        try:
            if ok:
                ok = False
                self._drain()
                self._write(BGZF_EOF)
                if self.index:  # (a refusal leaves through here: neither file appears)
                    bai = self._index_finish()
                    with open(bai_tmp, "wb") as fh:
                        fh.write(bai)
                ok = True
        finally:
            self.pool.shutdown(wait=True)
            self.fh.close()
            if self.idx is not None:
                _index_lib().bqsr_bam_index_destroy(self.idx)
                self.idx = None
            if ok:
                os.replace(self.tmp, self.path)
                if self.index:
                    os.replace(bai_tmp, self.path + ".bai")
            else:
                for p in (self.tmp, bai_tmp):
                    if os.path.exists(p):
                        os.remove(p)


PARQUET_ENCODERS = ("host", "device")


def _encoder_refusal(inp: str, adam_out: bool, compression: str) -> Optional[str]:
    """why -parquet_encoder device cannot serve this job (None: it can)"""
    if not adam_out:
        return "-parquet_encoder device applies to ADAM Parquet output only (not SAM or BAM)"
    if is_parquet(inp):
        return "-parquet_encoder device applies to SAM or BAM input (ADAM Parquet input keeps its own writer)"
    if compression == "zstd":
        return "-parquet_encoder device writes gzip, snappy or none (not zstd)"
    return None


class _AdamOut:
    """ADAM output (adamSave): part files of `part_reads` records each.
    encoder "device": the parts' data pages are built on the device
    (adam_pages.part_columns) and put together by a parquet_pages.PagesWriter
    -- the same part numbering, .partial / _SUCCESS / overwrite rules; page_rows
    overrides the rows per page (tests).  compressor "device": the encoder
    compresses the data pages (snappy) before they come down."""

    def __init__(self, path: str, compression: str, part_reads: int, overwrite: bool = False,
                 encoder: str = "host", page_rows: Optional[int] = None, device: int = 0, compressor: str = "host"):
        from .adam_save import ADAM_FIELDS, AdamWriter
        self.on_device = encoder == "device"
        self.compressor = compressor
        self.part_reads = part_reads
        self.page_rows = page_rows
        self.device = device
        self.enc = None  # the page encoder (made at the first emit: it needs the parse's context)
        if self.on_device:
            from .parquet_pages import PagesWriter
            self.w = PagesWriter(path, ADAM_FIELDS, compression, overwrite=overwrite, max_pending=2)
        else:
            self.w = AdamWriter(path, compression, overwrite=overwrite)

    def emit(self, i, sam, quals=None):
        """the ADAM columns with the apply's quals (no text rewrite)"""
        from .adam_save import header_info, set_quals
        if quals is not None:
            set_quals(sam, *quals)
        if not self.on_device:
            self.w.emit(sam, self.part_reads)
            return
        from . import adam_pages
        from .parquet_pages import Encoder
        if self.enc is None:
            self.enc = Encoder(sam.ctx, self.compressor)
        hdr = header_info(sam)
        n = sam.counts().n_reads
        for r0 in range(0, max(n, 1), max(1, self.part_reads)):  # (no reads: one part of the schema alone)
            m = min(self.part_reads, n - r0) if n else 0
            cols = adam_pages.part_columns(sam, self.enc, r0, m, hdr, self.w.compression, self.page_rows,
                                           self.device) if m else []
            self.w.add(cols, m)

    def close(self, ok: bool = True):
        try:
            self.w.close(ok)
        finally:
            if self.enc is not None:
                self.enc.close()

    def page_stats(self) -> Dict[str, object]:
        """measured: the page kernels' device-event ms, the encoded bytes downloaded, the files' bytes"""
        ms = dict(self.enc.ms) if self.enc is not None else {}
        return {"kernel_ms": ms, "bytes_downloaded": self.enc.bytes_down if self.enc is not None else 0,
                "file_bytes": self.w.file_bytes}


def transform(inp: str, out: str, mark_duplicates: bool = False, recalibrate: bool = False,
              dbsnp: Optional[str] = None, device: int = 0, partition_bytes: int = DEFAULT_PARTITION_BYTES,
              compression: str = "gzip", part_reads: int = 1 << 19, overwrite: bool = False,
              sort_reads: bool = False, bam_level: Optional[int] = None,
              bam_piece_reads: int = BAM_PIECE_READS, bam_compressor: Optional[str] = None,
              bam_index: bool = False, parquet_encoder: str = "host",
              page_rows: Optional[int] = None, parquet_compressor: str = "host", region: Optional[str] = None,
              bai: Optional[str] = None) -> Dict[str, float]:
    """Transform.run (cli/Transform.scala:62-97) over SAM or BAM input: the
    records parsed on the device (a BAM's records become SAM lines there),
    MarkDuplicates, BQSR, then adamSave (OUT.adam / .parquet / a directory:
    ADAMRecord Parquet part files, adam_save.py), BAM (OUT.bam, _BamOut:
    bam_level 0-9 (None: 6), records per encoded piece bam_piece_reads,
    bam_compressor "host" (None) or "device": the BGZF members deflated on
    the device, one level; bam_index: OUT.bam.bai beside it, built on the
    device, see _BamOut) or SAM text.  parquet_encoder "device": the ADAM part
    files' data pages encoded on the device (see the module doc and _AdamOut;
    page_rows: rows per page, for tests); parquet_compressor "device": those
    pages snappy-compressed on the device too (only with parquet_encoder
    "device" and compression "snappy").
    ADAM Parquet input goes through transform_parquet (Arrow reads it on the
    host).  sort_reads: the records sorted on the device before the save (see
    the module doc); the input must be one partition.  region, bai: BAM
    input read through its .bai index (inputs.SamInput): the job sees only the
    reads that overlap the region, in one partition; MarkDuplicates and BQSR
    work on what the region holds, so a mate outside it is absent, as if the
    input were the filtered file."""
    region = region_plan(inp, region, bai)  # before anything is read or created
    from .adam_save import is_adam_output
    bam_out = out.endswith(".bam")
    # ADAM output by name, or over an earlier adamSave directory (never just
    # because `out` is some existing directory: the sinks refuse that)
    adam_out = not bam_out and (out.endswith((".adam", ".parquet")) or is_adam_output(out))
    if parquet_encoder not in PARQUET_ENCODERS:
        raise ValueError("-parquet_encoder must be one of %s" % ", ".join(PARQUET_ENCODERS))
    if parquet_encoder == "device":  # before anything is read or created
        why = _encoder_refusal(inp, adam_out, compression)
        if why:
            raise ValueError(why)
    why = compressor_refusal(parquet_compressor, parquet_encoder, compression)  # before anything is read or created
    if why:
        raise ValueError(why)
    if bam_index and not bam_out:  # before anything is read
        raise ValueError(BAM_INDEX_REFUSAL)
    if bam_compressor is not None and not bam_out:  # before anything is read
        raise ValueError("-bam_compressor applies to BAM output only (an output name ending in .bam)")
    if bam_compressor is not None and bam_compressor not in BAM_COMPRESSORS:
        raise ValueError("-bam_compressor must be one of %s" % ", ".join(BAM_COMPRESSORS))
    if bam_compressor == "device" and bam_level is not None:
        raise ValueError(DEVICE_LEVEL_REFUSAL)
    if bam_out and is_parquet(inp):  # before anything is read
        raise ValueError("ADAM Parquet input cannot be written as BAM by transform (no SAM lines to encode): "
                         "python -m adam_amd.adam2sam writes it as BAM or SAM")
    if is_parquet(inp):
        return transform_parquet(inp, out, mark_duplicates, recalibrate, dbsnp, device, overwrite, sort_reads)
    if sort_reads:  # refused before any output file or parse exists
        with SamInput(inp, None, None, partition_bytes) as src:
            if src.n_partitions > 1:
                raise ValueError("-sort_reads needs the input in one partition; raise -partition_bytes")
    t0 = time.perf_counter()
    sink = (_BamOut(out, bam_level, bam_piece_reads, overwrite, bam_compressor or "host", bam_index) if bam_out
            else _AdamOut(out, compression, part_reads, overwrite, parquet_encoder, page_rows, device,
                          parquet_compressor) if adam_out
            else _SamOut(out, overwrite))
    try:
        ctx = bqsr.Context.get(device)
    except BaseException:
        sink.close(False)
        raise
    ok = False
    stats: Dict[str, float] = {}
    try:
        ph = _Phases()
        # (without a step that works across the whole input the records go through in one parse)
        with SamInput(inp, ctx, ph, partition_bytes if recalibrate or mark_duplicates or sort_reads else None,
                      region=region, bai=bai) as src:
            if src.n_partitions > 1:
                stats = _partitions(src.data, src.header, src.ranges, mark_duplicates, recalibrate, dbsnp, ctx, device,
                                    sink.emit)
            else:
                for sam, _ in src:
                    stats["reads"] = sam.counts().n_reads
                    stats.update(src.region_stats or {})
                    if mark_duplicates:
                        with ph("markdup"):
                            stats["duplicates"] = sam.mark_duplicates()
                    if recalibrate:
                        from .job import ResidentJob
                        snp = bqsr.SnpTable.from_vcf(dbsnp) if dbsnp else bqsr.SnpTable()
                        with ph("batch"):
                            job = ResidentJob(None, None, snp if snp.table else None, device, sam=sam)
                        try:
                            with ph("bqsr"):
                                job.step()
                            p = job._ptr
                            quals = (job.bh, p(job.out_qual), p(job.out_start), p(job.out_len), p(job.exc),
                                     job.n_exc, job.sp)
                            if sort_reads:  # the recalibrated text first: the apply's outputs are in input order
                                with ph("sort"):
                                    check(_capi.lib().bqsr_sam_rewrite_quals(ctx.handle, sam.h, *quals))
                                    sam.sort()
                                quals = None
                            with ph("emit"):
                                sink.emit(0, sam, quals)
                        finally:
                            job.close()
                    else:
                        if sort_reads:
                            with ph("sort"):  # (MarkDuplicates' FLAG bits go into the text there)
                                sam.sort()
                        with ph("emit"):
                            sink.emit(0, sam, None)
                stats["phases"] = ph.t
        ok = True
    finally:
        t1 = time.perf_counter()
        sink.close(ok)
        stats.setdefault("phases", {})["close"] = time.perf_counter() - t1
    if adam_out:
        stats["parts"] = sink.w.parts
        if ok and parquet_encoder == "device":
            stats["pages"] = sink.page_stats()
    if bam_out:
        stats["bam"] = sink.stats
    stats["seconds"] = time.perf_counter() - t0
    return stats


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="adam_amd.transform", description=__doc__.split("\n\n")[0])
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("-mark_duplicate_reads", action="store_true")
    ap.add_argument("-recalibrate_base_qualities", action="store_true")
    ap.add_argument("-dbsnp_sites", default=None)
    ap.add_argument("-sort_reads", action="store_true",
                    help="sort the records by reference position before the save (one partition)")
    ap.add_argument("-realignIndels", action="store_true")
    ap.add_argument("-coalesce", type=int, default=-1)
    ap.add_argument("-partition_bytes", type=int, default=DEFAULT_PARTITION_BYTES,
                    help="records per streamed partition, in bytes of SAM text")
    ap.add_argument("-parquet_compression", default="gzip", choices=("gzip", "snappy", "zstd", "none"),
                    help="ADAM output: the part files' codec (adamSave's default: GZIP)")
    ap.add_argument("-part_reads", type=int, default=1 << 19, help="ADAM output: records per part file")
    ap.add_argument("-parquet_encoder", default="host", choices=PARQUET_ENCODERS,
                    help="ADAM output from SAM or BAM input: where the part files' data pages are encoded (device: "
                         "adam_amd/adam_pages.py; gzip, snappy or none)")
    ap.add_argument("-parquet_compressor", default="host", choices=PARQUET_COMPRESSORS,
                    help="with -parquet_encoder device and -parquet_compression snappy: where the data pages are "
                         "compressed (device: adam_amd/csrc/snappy_pages.hip)")
    ap.add_argument("-bam_compression_level", type=int, default=None, choices=range(10), metavar="N",
                    help="BAM output (OUTPUT.bam): the BGZF members' DEFLATE level, 0-9 (0: stored; default 6, "
                         "zlib's and samtools'); the host compressor's")
    ap.add_argument("-bam_compressor", default=None, choices=BAM_COMPRESSORS,
                    help="BAM output: who deflates the BGZF members: host threads (default) or the device "
                         "(one level: not together with -bam_compression_level)")
    ap.add_argument("-bam_index", action="store_true",
                    help="BAM output: write OUTPUT.bam.bai beside it, built on the device (the output must be in "
                         "coordinate order)")
    ap.add_argument("-overwrite", action="store_true",
                    help="replace an existing output (a file, or a directory of ADAM part files only)")
    add_region_arguments(ap)
    a = ap.parse_args(argv)
    if a.realignIndels or a.coalesce != -1:
        ap.error("-coalesce / -realignIndels are outside this build")
    if a.bam_compressor is not None and not a.output.endswith(".bam"):
        ap.error("-bam_compressor applies to BAM output only (an output name ending in .bam)")
    if a.bam_compressor == "device" and a.bam_compression_level is not None:
        ap.error(DEVICE_LEVEL_REFUSAL)
    if a.bam_index and not a.output.endswith(".bam"):
        ap.error(BAM_INDEX_REFUSAL)
    why = compressor_refusal(a.parquet_compressor, a.parquet_encoder, a.parquet_compression)
    if why:
        ap.error(why)
    try:
        a.region = region_plan(a.input, a.region, a.bai)
    except (ValueError, OSError) as e:
        ap.error(str(e))
    t0 = time.perf_counter()
    st = transform(a.input, a.output, a.mark_duplicate_reads, a.recalibrate_base_qualities, a.dbsnp_sites,
                   partition_bytes=a.partition_bytes, compression=a.parquet_compression, part_reads=a.part_reads,
                   overwrite=a.overwrite, sort_reads=a.sort_reads, bam_level=a.bam_compression_level,
                   bam_compressor=a.bam_compressor, bam_index=a.bam_index, parquet_encoder=a.parquet_encoder,
                   parquet_compressor=a.parquet_compressor, region=a.region, bai=a.bai)
    report(st, t0)
    return 0


if __name__ == "__main__":
    sys.exit(main())
