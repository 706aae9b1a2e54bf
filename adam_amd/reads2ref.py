"""`adam reads2ref` on the device: reads to ADAMPileup records.

The reference's Reads2Ref (adam-cli/.../cli/Reads2Ref.scala:53-75) loads reads
with ``adamLoad`` and LocusPredicate, maps every read through
Reads2PileupProcessor.readToPileups (adam-core/.../rdd/
Reads2PileupProcessor.scala:34-197) and saves the ADAMPileup records
(adam-format/.../avro/adam.avdl:99-128) with adamSave.  Here the expansion
runs on the GPU (include/adam_sam.h ``bqsr_sam_pileup_*`` /
``bqsr_arrow_pileup_*``, adam_amd/csrc/pileup.hip): a count / validate pass
per read, a scan, and an emit pass with a lane per output row; the row-level
columns come back as Arrow buffers, and the read-level ones (readName,
referenceName, the recordGroup* fields) become Arrow dictionary arrays whose
indices are gathered through the device's ``read`` column -- no string is
expanded row by row.

What is kept from the reference, quirks included:

* LocusPredicate (readMapped, primaryAlignment, !failedVendorQualityChecks,
  !duplicateRead; a null fails) filters **Parquet input only**
  (AdamContext.scala:318-332 ignores the predicate for .sam / .bam): every
  SAM / BAM record is converted.
* A read without CIGAR or MD gives no pileups.  Where readToPileups throws
  the job fails with the first such read in input order
  (:class:`_capi.BQSRError`, ``.read``): NULL_FIELD, MD_PARSE, or PILEUP for
  everything thrown inside the CIGAR walk -- a sequence char outside the Base
  enum, sequence or quals shorter than the CIGAR, CIGAR and MD disagreeing,
  and any pileup of a read whose readMapped is false, which on SAM input
  includes FLAG-0 records (quirk Q2).  No output appears then.
* Reads in input order, a read's pileups in reverse walk order.
* ``-mapq N`` is parsed and never read, as in the reference.
* ``-aggregate`` is refused: PileupAggregator joins read names in Spark's
  shuffle order, so the reference does not define its result.

    python -m adam_amd.reads2ref INPUT.{sam,bam,adam} OUTPUT.adam [-mapq N] [-aggregate]
        [-parquet_compression gzip|snappy|none] [-part_reads N] [-partition_bytes N] [-overwrite]
"""
from __future__ import annotations

import argparse
import ctypes
import sys
import time
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _capi, adam_save, bqsr
from ._capi import check, dblp, i32, i64, vp
from .adam_save import (BASES, PILEUP_DICT_COLS, PILEUP_FIELDS, PILEUP_STATS_COLS, RG_TAGS, AdamHost, AdamSizes,
                        AdamWriter, HeaderInfo, _pinned, check_out, header_info, pileup_schema)
from .inputs import DEFAULT_PARTITION_BYTES, Phases, SamInput, is_parquet, rebased, report

# Reads per part file.  A read gives about as many rows as it has bases and a
# row takes 54 bytes of device columns and as many of pinned host memory
# (then Arrow's encoder works from those buffers): 131072 reads of 150 bases
# are ~20M rows, ~1.1 GB on either side, with the next part's buffers
# alongside while host threads encode -- small beside HBM and host memory,
# large enough that a part file's fixed costs do not show, and far from the
# 2^31 - 1 rows one call takes (reads of up to 16 kb).
DEFAULT_PART_READS = 1 << 17

LOCUS_COLUMNS = ("readMapped", "primaryAlignment", "failedVendorQualityChecks", "duplicateRead")
# the ADAMRecord columns reads2ref reads from Parquet
PROJECTION = ("referenceName", "referenceId", "start", "mapq", "readName", "sequence", "cigar", "qual",
              "readNegativeStrand", "mismatchingPositions", "recordGroupSequencingCenter", "recordGroupDescription",
              "recordGroupRunDateEpoch", "recordGroupFlowOrder", "recordGroupKeySequence", "recordGroupLibrary",
              "recordGroupPredictedMedianInsertSize", "recordGroupPlatform", "recordGroupPlatformUnit",
              "recordGroupSample") + LOCUS_COLUMNS
# the fields copied from the read, by Arrow type
_READ_LEVEL = [(n, k) for n, k in PILEUP_FIELDS if n in ("referenceName", "referenceId") or n.startswith("recordGroup")]


class PileupSizes(ctypes.Structure):
    _fields_ = [("n_reads", ctypes.c_int64), ("n_rows", ctypes.c_int64), ("bitmap_words", ctypes.c_int64)]


# bqsr_pileup_host, in order: (field, dtype, per row / per bitmap word)
_HOST = (("read", np.int32), ("position", np.int64), ("range_offset", np.int32), ("range_length", np.int32),
         ("reference_base", np.uint8), ("read_base", np.uint8), ("sanger_quality", np.int32),
         ("map_quality", np.int32), ("num_soft_clipped", np.int32), ("num_reverse_strand", np.int32),
         ("read_start", np.int64), ("read_end", np.int64), ("range_valid", np.uint64),
         ("reference_base_valid", np.uint64), ("read_base_valid", np.uint64), ("map_quality_valid", np.uint64))


class PileupHost(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n, _ in _HOST]


KERNELS = ("count", "emit")
_SIG = {
    "bqsr_sam_pileup_prepare": (ctypes.c_int, [vp, vp, i64, i64, vp, ctypes.POINTER(PileupSizes)]),
    "bqsr_sam_pileup_columns": (ctypes.c_int, [vp, vp, ctypes.POINTER(PileupHost), vp]),
    "bqsr_arrow_pileup_prepare": (ctypes.c_int, [vp, vp, i64, i64, vp, vp, vp, i32, vp, ctypes.POINTER(PileupSizes)]),
    "bqsr_arrow_pileup_columns": (ctypes.c_int, [vp, vp, ctypes.POINTER(PileupHost), vp]),
    "bqsr_pileup_kernel_times": (ctypes.c_int, [dblp, dblp]),
}


def _lib():
    return _capi.bind(_capi.lib(), _SIG)


def kernel_times():
    """(count ms, emit ms): the two kernels of this thread's last prepare /
    columns calls, by device events (measurement only)"""
    return tuple(_capi.stage_times(_lib().bqsr_pileup_kernel_times, KERNELS).values())


def _host_columns(n_rows: int):
    """(PileupHost, arrays): the host buffers of n_rows rows, carved from one
    pinned block (the copies run at the link's rate)"""
    W = (n_rows + 63) // 64
    sizes = [((max(1, W if dt == np.uint64 else n_rows) * np.dtype(dt).itemsize + 63) // 64) * 64 for _, dt in _HOST]
    block = _pinned(sum(sizes))
    H = PileupHost()
    arrays = {}
    pos = 0
    for (name, dt), nb in zip(_HOST, sizes):
        a = block[pos:pos + nb].view(dt)[:max(1, W if dt == np.uint64 else n_rows)]
        pos += nb
        arrays[name] = a
        setattr(H, name, a.ctypes.data)
    return H, arrays


class _ReadLevel:
    """What a range's pileups copy from their reads: readName (an Arrow
    string array, one entry per read) and, per read-level field, (codes,
    valid, values): the read's index into `values`, None entries null."""

    def __init__(self, read_name, coded: Dict[str, tuple]):
        self.read_name = read_name
        self.coded = coded


def _table(n_rows: int, a: Dict[str, np.ndarray], rl: _ReadLevel):
    """The ADAMPileup table of the device's columns `a` (zero-copy views of
    the pinned buffers) and the read-level values gathered through `read`."""
    import pyarrow as pa
    if n_rows == 0:
        return pileup_schema().empty_table()
    n = n_rows
    pb = pa.py_buffer
    read = a["read"][:n]

    def ints(name, typ, valid=None):
        return pa.Array.from_buffers(typ, n, [None if valid is None else pb(a[valid]), pb(a[name][:n])])

    def base(name):
        ind = pa.Array.from_buffers(pa.int8(), n, [pb(a[name + "_valid"]), pb(a[name][:n])])
        return pa.DictionaryArray.from_arrays(ind, pa.array(BASES, pa.string()), safe=False)

    cols = {
        "position": ints("position", pa.int64()),
        "rangeOffset": ints("range_offset", pa.int32(), "range_valid"),
        "rangeLength": ints("range_length", pa.int32(), "range_valid"),
        "referenceBase": base("reference_base"),
        "readBase": base("read_base"),
        "sangerQuality": ints("sanger_quality", pa.int32()),
        "mapQuality": ints("map_quality", pa.int32(), "map_quality_valid"),
        "numSoftClipped": ints("num_soft_clipped", pa.int32()),
        "numReverseStrand": ints("num_reverse_strand", pa.int32()),
        "countAtPosition": pa.array(np.ones(n, np.int32)),
        "readStart": ints("read_start", pa.int64()),
        "readEnd": ints("read_end", pa.int64()),
    }
    # readName: the reads' names are the dictionary, `read` the indices
    names = rl.read_name
    if names.null_count:
        ok = np.asarray(names.is_valid().to_numpy(zero_copy_only=False), bool)[read]
        ind = pa.array(read, pa.int32(), mask=~ok)
        names = names.fill_null("")
    else:
        ind = pa.Array.from_buffers(pa.int32(), n, [None, pb(read)])
    cols["readName"] = pa.DictionaryArray.from_arrays(ind, names, safe=False)
    t = {"string": pa.string(), "int32": pa.int32(), "int64": pa.int64()}
    gathered: Dict[int, tuple] = {}
    for name, kind in _READ_LEVEL:
        codes, valid, values = rl.coded[name]
        has = np.asarray([v is not None for v in values], bool)
        if not has.any():
            cols[name] = pa.nulls(n, t[kind])
            continue
        key = id(codes)
        if key not in gathered:  # one gather per index column (referenceId / recordGroupId), shared
            gathered[key] = (codes[read], valid[read])
        c, v = gathered[key]
        ok = v & has[np.clip(c, 0, len(values) - 1)]
        ind = pa.array(np.where(ok, c, 0).astype(np.int32), mask=None if ok.all() else ~ok)
        dic = pa.array([x if x is not None else ("" if kind == "string" else 0) for x in values], t[kind])
        cols[name] = pa.DictionaryArray.from_arrays(ind, dic, safe=False)
    return pa.table([cols[name] for name, _ in PILEUP_FIELDS], names=[name for name, _ in PILEUP_FIELDS])


def _sam_read_level(sam, r0: int, n: int, hdr: HeaderInfo, stream=None) -> _ReadLevel:
    """readName, referenceId and recordGroupId of reads [r0, r0 + n) from the
    device's ADAM columns (bqsr_sam_adam_*); the rest by index from the header"""
    import pyarrow as pa
    L = adam_save._lib()
    sz = AdamSizes()
    check(L.bqsr_sam_adam_prepare(sam.ctx.handle, sam.h, r0, n, stream, ctypes.byref(sz)))
    W = sz.bitmap_words
    off = np.zeros(n + 1, np.int32)
    data = np.zeros(max(1, sz.str_bytes[0]), np.uint8)
    i32 = [np.zeros(max(1, n), np.int32) for _ in range(2)]
    valid = [np.zeros(max(1, W), np.uint64) for _ in range(2)]
    H = AdamHost()
    H.str_offsets[0] = off.ctypes.data
    H.str_bytes[0] = data.ctypes.data if sz.str_bytes[0] else None
    H.i32[0], H.int_valid[0] = i32[0].ctypes.data, valid[0].ctypes.data  # referenceId
    H.i32[3], H.int_valid[3] = i32[1].ctypes.data, valid[1].ctypes.data  # recordGroupId
    check(L.bqsr_sam_adam_columns(sam.ctx.handle, sam.h, ctypes.byref(H), stream))
    names = pa.StringArray.from_buffers(n, pa.py_buffer(off), pa.py_buffer(data[:sz.str_bytes[0]]))
    bits = [np.unpackbits(v.view(np.uint8), count=n, bitorder="little").astype(bool) for v in valid]
    ref = (i32[0][:n], bits[0])
    rg = (i32[1][:n], bits[1])
    coded = {"referenceName": ref + ([r["SN"] for r in hdr.sq],),
             "referenceId": ref + (list(range(len(hdr.sq))),),
             "recordGroupRunDateEpoch": rg + (hdr.rg_column("DT", "date"),),
             "recordGroupPredictedMedianInsertSize": rg + (hdr.rg_column("PI", "int"),)}
    for name, key in RG_TAGS:
        coded[name] = rg + (hdr.rg_column(key),)
    return _ReadLevel(names, coded)


def sam_pileups(sam, r0: int = 0, n: Optional[int] = None, hdr: Optional[HeaderInfo] = None, stream=None):
    """The ADAMPileup table (pyarrow) of reads [r0, r0 + n) of a sam.SamText
    (every read: SAM / BAM input is not filtered)."""
    L = _lib()
    total = sam.counts().n_reads
    n = total - r0 if n is None else n
    sz = PileupSizes()
    check(L.bqsr_sam_pileup_prepare(sam.ctx.handle, sam.h, r0, n, stream, ctypes.byref(sz)))
    if sz.n_rows == 0:
        return _table(0, {}, None)
    H, arrays = _host_columns(sz.n_rows)
    check(L.bqsr_sam_pileup_columns(sam.ctx.handle, sam.h, ctypes.byref(H), stream))
    return _table(sz.n_rows, arrays, _sam_read_level(sam, r0, n, hdr or header_info(sam), stream))


def _arrow_read_level(table, r0: int, n: int) -> _ReadLevel:
    import pyarrow as pa
    import pyarrow.compute as pc
    have = set(table.column_names)
    t = {"string": pa.string(), "int32": pa.int32(), "int64": pa.int64()}
    sl = table.slice(r0, n)

    def col(name, typ):
        if name not in have:
            return pa.nulls(n, typ)
        c = sl.column(name).combine_chunks()
        if isinstance(c, pa.ChunkedArray):
            c = pa.concat_arrays(c.chunks) if c.num_chunks else pa.nulls(0, typ)
        return c if c.type == typ else c.cast(typ)

    coded = {}
    for name, kind in _READ_LEVEL:
        d = col(name, t[kind]).dictionary_encode()
        codes = np.asarray(pc.fill_null(d.indices, 0).to_numpy(zero_copy_only=False), np.int32)
        valid = np.asarray(d.indices.is_valid().to_numpy(zero_copy_only=False), bool)
        coded[name] = (codes, valid, d.dictionary.to_pylist())
    return _ReadLevel(col("readName", pa.string()), coded)


def _arrow_prepare(reads, r0: int, n: int, stream=None) -> PileupSizes:
    """bqsr_arrow_pileup_prepare over reads [r0, r0 + n) of a parquet.ArrowReads"""
    import pyarrow as pa
    L = _lib()
    table = reads.table
    sz = PileupSizes()
    if not getattr(reads, "_mapq_sent", False):
        # mapq is not among bqsr_arrow_chunk's columns: handed over here, once per handle
        keep, lens, vals, valids = [], [], [], []
        if "mapq" in table.column_names:
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
        a_len = (ctypes.c_int64 * max(1, k))(*lens)
        a_val = (ctypes.c_void_p * max(1, k))(*vals)
        a_ok = (ctypes.c_void_p * max(1, k))(*valids)
        check(L.bqsr_arrow_pileup_prepare(reads.ctx.handle, reads.h, r0, n, a_len, a_val, a_ok, k, stream,
                                          ctypes.byref(sz)))
        del keep
        reads._mapq_sent = True
    else:
        check(L.bqsr_arrow_pileup_prepare(reads.ctx.handle, reads.h, r0, n, None, None, None, 0, stream,
                                          ctypes.byref(sz)))
    return sz


def arrow_pileups(reads, r0: int = 0, n: Optional[int] = None, stream=None):
    """The ADAMPileup table of reads [r0, r0 + n) of a parquet.ArrowReads
    (its table as given: apply :func:`locus_filter` before the upload)."""
    L = _lib()
    table = reads.table
    n = reads.n_reads - r0 if n is None else n
    sz = _arrow_prepare(reads, r0, n, stream)
    if sz.n_rows == 0:
        return _table(0, {}, None)
    H, arrays = _host_columns(sz.n_rows)
    check(L.bqsr_arrow_pileup_columns(reads.ctx.handle, reads.h, ctypes.byref(H), stream))
    return _table(sz.n_rows, arrays, _arrow_read_level(table, r0, n))


def locus_filter(table):
    """LocusPredicate (predicates/LocusPredicate.scala) over an Arrow table of
    ADAMRecords: readMapped, primaryAlignment, !failedVendorQualityChecks,
    !duplicateRead; a null -- or an absent column -- fails."""
    import pyarrow as pa
    import pyarrow.compute as pc
    mask = None
    for name, want in zip(LOCUS_COLUMNS, (True, True, False, False)):
        if name not in table.column_names:
            return table.slice(0, 0)
        m = pc.fill_null(pc.equal(table.column(name).cast(pa.bool_()), want), False)
        mask = m if mask is None else pc.and_(mask, m)
    return table.filter(mask)


def _reads2ref(inp: str, out: str, compression: str, part_reads: int, partition_bytes: int, overwrite: bool,
               device: int, writer_args: Optional[dict] = None) -> Dict[str, object]:
    check_out(out, overwrite, True)
    ctx = bqsr.Context.get(device)
    ph = Phases()
    part_reads = max(1, int(part_reads))
    stats: Dict[str, object] = {"reads": 0, "pileups": 0}
    W = AdamWriter(out, compression, overwrite=overwrite, dict_cols=PILEUP_DICT_COLS, stats_cols=PILEUP_STATS_COLS,
                   huffman_cols=(), max_pending=2, **(writer_args or {}))
    ok = False
    try:
        def emit(make_table, n, base):
            for r0 in range(0, n, part_reads):
                try:
                    with ph("pileups"):
                        t = make_table(r0, min(part_reads, n - r0))
                except _capi.BQSRError as e:
                    raise rebased(e, base) from None
                if t.num_rows:
                    stats["pileups"] += t.num_rows
                    with ph("write"):
                        W.add(t)

        if is_parquet(inp):
            from . import parquet as P
            with ph("read"):
                table = locus_filter(P.read_table(inp, columns=PROJECTION))
            with ph("parse"):
                A = P.ArrowReads(table, ctx)
            try:
                emit(lambda r0, n: arrow_pileups(A, r0, n), table.num_rows, 0)
            finally:
                A.close()
            stats["reads"] = table.num_rows
        else:
            with SamInput(inp, ctx, ph, partition_bytes) as src:
                stats["partitions"] = src.n_partitions
                for sam, base in src:
                    hdr = header_info(sam)
                    n = sam.counts().n_reads
                    emit(lambda r0, m: sam_pileups(sam, r0, m, hdr), n, base)
                    stats["reads"] = base + n
        if W.parts == 0:  # no pileups at all: one empty part file carries the schema
            W.add(pileup_schema().empty_table())
        ok = True
    finally:
        with ph("close"):
            W.close(ok)
    stats["parts"] = W.parts
    stats["phases"] = ph.t
    return stats


def reads2ref(inp: str, out: str, aggregate: bool = False, min_mapq: int = 30, compression: str = "gzip",
              part_reads: int = DEFAULT_PART_READS, partition_bytes: Optional[int] = None, overwrite: bool = False,
              device: int = 0) -> Dict[str, object]:
    """`adam reads2ref`: the reads of a SAM, BAM or ADAMRecord Parquet input
    as ADAMPileup Parquet part files under `out` (which appears only when the
    job succeeds; an existing one is refused unless overwrite, and then only
    an earlier part-file directory is replaced).  min_mapq is accepted and
    ignored, as the reference never reads its -mapq.  part_reads: reads per
    part file (:data:`DEFAULT_PART_READS`); partition_bytes: SAM text per
    streamed partition (inputs.DEFAULT_PARTITION_BYTES).  Returns the
    job's statistics."""
    if aggregate:
        raise ValueError("-aggregate is outside this build: PileupAggregator joins read names in Spark's shuffle "
                         "order, so the reference itself does not define its result")
    int(min_mapq)  # (checked to be a number, then unused: Reads2Ref.scala parses -mapq and never reads it)
    return _reads2ref(inp, out, compression, part_reads,
                      DEFAULT_PARTITION_BYTES if partition_bytes is None else partition_bytes, overwrite, device)


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="adam_amd.reads2ref", description=__doc__.split("\n\n")[0])
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("-mapq", type=int, default=30,
                    help="accepted and ignored: the reference parses it and never reads it")
    ap.add_argument("-aggregate", action="store_true", help="refused (see the module's notes)")
    ap.add_argument("-parquet_compression", default="gzip", choices=("gzip", "snappy", "none"))
    ap.add_argument("-part_reads", type=int, default=DEFAULT_PART_READS, help="reads per part file")
    ap.add_argument("-partition_bytes", type=int, default=DEFAULT_PARTITION_BYTES,
                    help="SAM text per streamed partition, in bytes")
    ap.add_argument("-overwrite", action="store_true")
    a = ap.parse_args(argv)
    if a.aggregate:
        ap.error("-aggregate is outside this build (PileupAggregator's result depends on Spark's shuffle order)")
    t0 = time.perf_counter()
    st = reads2ref(a.input, a.output, False, a.mapq, a.parquet_compression, a.part_reads, a.partition_bytes,
                   a.overwrite)
    report(st, t0)
    return 0


if __name__ == "__main__":
    sys.exit(main())
