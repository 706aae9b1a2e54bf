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
        [-parquet_encoder host|device] [-parquet_compressor host|device]

``-parquet_encoder device`` builds the part files' data pages on the GPU from
the columns the emit pass leaves there (adam_amd/parquet_pages.py): only the
encoded pages are downloaded; the host adds page headers, dictionary pages,
the codec and the footer.  The default, ``host``, is Arrow's writer.
``-parquet_compressor device`` (only with ``-parquet_encoder device
-parquet_compression snappy``; refused otherwise before anything is read or
created) compresses those data pages on the GPU too
(adam_amd/csrc/snappy_pages.hip): the raw bodies are not downloaded.
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
from .inputs import DEFAULT_PARTITION_BYTES, Phases, SamInput, add_region_arguments, is_parquet, rebased, region_plan, report
from .parquet_pages import COMPRESSORS, compressor_refusal

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
    "bqsr_sam_pileup_device_columns": (ctypes.c_int, [vp, vp, ctypes.POINTER(PileupHost), vp]),
    "bqsr_arrow_pileup_device_columns": (ctypes.c_int, [vp, vp, ctypes.POINTER(PileupHost), vp]),
    "bqsr_sam_pileup_read_spans": (ctypes.c_int, [vp, vp, vp, vp, vp]),
    "bqsr_arrow_pileup_read_spans": (ctypes.c_int, [vp, vp, vp, vp, vp]),
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


# ---- -parquet_encoder device: the part files' data pages built on the GPU ----
# (adam_amd/parquet_pages.py; the columns stay on the device, only the encoded pages come back)

# the int32 columns small enough for a dense-range dictionary [min, max], index = value - min: (field, device
# column, validity bitmap)
_SMALL_INTS = (("rangeOffset", "range_offset", "range_valid"), ("rangeLength", "range_length", "range_valid"),
               ("sangerQuality", "sanger_quality", None), ("mapQuality", "map_quality", "map_quality_valid"),
               ("numSoftClipped", "num_soft_clipped", None), ("numReverseStrand", "num_reverse_strand", None))


# readStart and readEnd with the device encoder, by codec: "dictionary" -- one entry per read of the part
# (duplicates are legal), the `read` column as indices, the stream readName already has -- or "plain" int64 like
# position.  Measured on the 2M-read run: the dictionary form is the faster under every codec and the
# smaller under snappy; under gzip, which folds PLAIN's runs of one value to almost nothing, it is 12 % larger in
# all, so gzip -- chosen for size -- keeps PLAIN.
READ_SPANS = {"gzip": "plain", "snappy": "dictionary", "none": "dictionary"}


def _page_columns(enc, D: PileupHost, n_rows: int, n_reads: int, rl: _ReadLevel, spans, page_rows: int, device: int,
                  stream=None):
    """The 25 parquet_pages.Column of a part from the device columns D (their
    device addresses, bqsr_*_pileup_device_columns): what :func:`_table`
    builds on the host, as descriptors.  spans: the reads' (readStart,
    readEnd) arrays (bqsr_*_pileup_read_spans), or None to write the two
    columns PLAIN."""
    import torch

    from . import parquet_pages as PP
    n = n_rows
    dev = torch.device("cuda", device)
    held = []  # the uploaded read-level tables, alive until the last encode

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
        held.append(t)
        return t.data_ptr()

    def desc(kind, src, width, src_n=n, **kw):
        return PP.ParquetColumn(kind=kind, src_width=width, src=getattr(D, src) if isinstance(src, str) else src,
                                src_n=src_n, gather=kw.get("gather"), remap=kw.get("remap"),
                                remap_n=kw.get("remap_n", 0), bit_width=kw.get("bit_width", 0), base=kw.get("base", 0),
                                validity=getattr(D, kw["validity"]) if kw.get("validity") else None)

    def encode(d):
        return enc.encode(d, n, page_rows, stream)

    cols = {}
    plain64 = [("position", "position")]
    if spans is None:
        plain64 += [("readStart", "read_start"), ("readEnd", "read_end")]
    for name, src in plain64:
        cols[name] = PP.Column(name, "int64", encode(desc(PP.PLAIN_INT64, src, 8)))
    bases = PP.plain_strings(BASES)
    for name, src in (("referenceBase", "reference_base"), ("readBase", "read_base")):
        d = desc(PP.DICT_INDEX, src, 1, bit_width=PP.bit_width(len(BASES)), validity=src + "_valid")
        cols[name] = PP.Column(name, "string", encode(d), bases)
    for name, src, valid in _SMALL_INTS:
        cols[name] = PP.small_int_column(enc, name, desc(PP.PLAIN_INT32, src, 4, validity=valid), n, page_rows, stream)
    # countAtPosition, the constant 1: a one-entry dictionary, every index 0 -- any byte column mapped through a
    # table of zeros
    zeros = up(np.zeros(256, np.int32))
    d = desc(PP.DICT_INDEX, "read_base", 1, remap=zeros, remap_n=256, bit_width=1)
    cols["countAtPosition"] = PP.Column("countAtPosition", "int32", encode(d), PP.plain_ints([1], "int32"))
    # readName: the part's names are the dictionary, `read` the indices
    names = rl.read_name
    kw = {}
    if names.null_count:
        ok = np.asarray(names.is_valid().to_numpy(zero_copy_only=False), bool)
        kw = dict(remap=up(np.where(ok, np.arange(n_reads), -1)), remap_n=n_reads)
        names = names.fill_null("")
    named = encode(desc(PP.DICT_INDEX, "read", 4, bit_width=PP.bit_width(n_reads), **kw))
    cols["readName"] = PP.Column("readName", "string", named, PP.plain_string_array(names))
    if spans is not None:  # the same index stream (when no name is null): encoded and compressed once
        by_read = encode(desc(PP.DICT_INDEX, "read", 4, bit_width=PP.bit_width(n_reads))) if kw else named
        for name, values in zip(("readStart", "readEnd"), spans):
            cols[name] = PP.Column(name, "int64", by_read, PP.plain_ints(values, "int64"))
    # the read-level fields: the read's code (-1: null) gathered through `read`, mapped through the field's
    # code -> index table, in which an entry without a value is -1; equal index streams are encoded once
    codes_dev: Dict[int, int] = {}
    streams: Dict[tuple, object] = {}
    for name, kind in _READ_LEVEL:
        codes, valid, values = rl.coded[name]
        if id(codes) not in codes_dev:
            codes_dev[id(codes)] = up(np.where(valid, codes, -1))
        has = np.asarray([v is not None for v in values], bool)
        remap = np.where(has, np.arange(len(values)), -1).astype(np.int32) if len(values) else np.full(1, -1, np.int32)
        key = (id(codes), remap.tobytes())
        if key not in streams:
            d = desc(PP.DICT_INDEX, codes_dev[id(codes)], 4, src_n=n_reads, gather=D.read, remap=up(remap),
                     remap_n=len(remap), bit_width=PP.bit_width(len(remap)))
            streams[key] = encode(d)
        fill = "" if kind == "string" else 0
        entries = [fill if v is None else v for v in values] or [fill]
        dic = PP.plain_strings(entries) if kind == "string" else PP.plain_ints(entries, kind)
        cols[name] = PP.Column(name, kind, streams[key], dic)
    del held
    return [cols[name] for name, _ in PILEUP_FIELDS]


def _read_spans(call, ctx_handle, handle, n: int, form: str, stream=None):
    """(readStart, readEnd) per read of the prepared range; None when the form is "plain" """
    if form != "dictionary":
        return None
    spans = np.zeros((2, max(1, n)), np.int64)
    check(call(ctx_handle, handle, spans[0].ctypes.data, spans[1].ctypes.data, stream))
    return spans[0, :n], spans[1, :n]


def sam_pileup_pages(sam, enc, r0: int, n: int, hdr: HeaderInfo, page_rows: int, device: int = 0, stream=None,
                     read_spans: str = "dictionary"):
    """(rows, parquet_pages columns or None when there is no row) of reads
    [r0, r0 + n) of a sam.SamText, the pages encoded on the device"""
    L = _lib()
    sz = PileupSizes()
    check(L.bqsr_sam_pileup_prepare(sam.ctx.handle, sam.h, r0, n, stream, ctypes.byref(sz)))
    if sz.n_rows == 0:
        return 0, None
    D = PileupHost()
    check(L.bqsr_sam_pileup_device_columns(sam.ctx.handle, sam.h, ctypes.byref(D), stream))
    rl = _sam_read_level(sam, r0, n, hdr, stream)
    spans = _read_spans(L.bqsr_sam_pileup_read_spans, sam.ctx.handle, sam.h, n, read_spans, stream)
    return sz.n_rows, _page_columns(enc, D, sz.n_rows, n, rl, spans, page_rows, device, stream)


def arrow_pileup_pages(reads, enc, r0: int, n: int, page_rows: int, device: int = 0, stream=None,
                       read_spans: str = "dictionary"):
    """the same for reads [r0, r0 + n) of a parquet.ArrowReads"""
    L = _lib()
    sz = _arrow_prepare(reads, r0, n, stream)
    if sz.n_rows == 0:
        return 0, None
    D = PileupHost()
    check(L.bqsr_arrow_pileup_device_columns(reads.ctx.handle, reads.h, ctypes.byref(D), stream))
    rl = _arrow_read_level(reads.table, r0, n)
    spans = _read_spans(L.bqsr_arrow_pileup_read_spans, reads.ctx.handle, reads.h, n, read_spans, stream)
    return sz.n_rows, _page_columns(enc, D, sz.n_rows, n, rl, spans, page_rows, device, stream)


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
               device: int, writer_args: Optional[dict] = None, parquet_encoder: str = "host",
               page_rows: Optional[int] = None, parquet_compressor: str = "host", region: Optional[str] = None,
               bai: Optional[str] = None) -> Dict[str, object]:
    if parquet_encoder not in ("host", "device"):
        raise ValueError("parquet_encoder is 'host' or 'device'")
    why = compressor_refusal(parquet_compressor, parquet_encoder, compression)  # before anything is read or created
    if why:
        raise ValueError(why)
    region = region_plan(inp, region, bai)  # (refused before anything is read or created)
    on_device = parquet_encoder == "device"
    check_out(out, overwrite, True)
    ctx = bqsr.Context.get(device)
    ph = Phases()
    part_reads = max(1, int(part_reads))
    stats: Dict[str, object] = {"reads": 0, "pileups": 0}
    enc = None
    if on_device:
        from . import parquet_pages as PP
        page_rows = PP.DEFAULT_PAGE_ROWS if page_rows is None else int(page_rows)
        spans = READ_SPANS[compression or "none"]
        W = PP.PagesWriter(out, PILEUP_FIELDS, compression, overwrite=overwrite, max_pending=2, **(writer_args or {}))
    else:
        W = AdamWriter(out, compression, overwrite=overwrite, dict_cols=PILEUP_DICT_COLS,
                       stats_cols=PILEUP_STATS_COLS, huffman_cols=(), max_pending=2, **(writer_args or {}))
    ok = False
    try:
        if on_device:
            enc = PP.Encoder(ctx, parquet_compressor)

        def emit(make_table, make_pages, n, base):
            for r0 in range(0, n, part_reads):
                m = min(part_reads, n - r0)
                try:
                    with ph("pileups"):
                        if on_device:
                            rows, cols = make_pages(r0, m)
                        else:
                            t = make_table(r0, m)
                            rows = t.num_rows
                except _capi.BQSRError as e:
                    raise rebased(e, base) from None
                if rows:
                    stats["pileups"] += rows
                    with ph("write"):
                        if on_device:
                            W.add(cols, rows)
                        else:
                            W.add(t)

        if is_parquet(inp):
            from . import parquet as P
            with ph("read"):
                table = locus_filter(P.read_table(inp, columns=PROJECTION))
            with ph("parse"):
                A = P.ArrowReads(table, ctx)
            try:
                emit(lambda r0, n: arrow_pileups(A, r0, n),
                     lambda r0, n: arrow_pileup_pages(A, enc, r0, n, page_rows, device, read_spans=spans),
                     table.num_rows, 0)
            finally:
                A.close()
            stats["reads"] = table.num_rows
        else:
            with SamInput(inp, ctx, ph, partition_bytes, region=region, bai=bai) as src:
                stats["partitions"] = src.n_partitions
                for sam, base in src:
                    stats.update(src.region_stats or {})
                    hdr = header_info(sam)
                    n = sam.counts().n_reads
                    emit(lambda r0, m: sam_pileups(sam, r0, m, hdr),
                         lambda r0, m: sam_pileup_pages(sam, enc, r0, m, hdr, page_rows, device, read_spans=spans),
                         n, base)
                    stats["reads"] = base + n
        if W.parts == 0:  # no pileups at all: one empty part file carries the schema
            if on_device:
                W.add([], 0)
            else:
                W.add(pileup_schema().empty_table())
        ok = True
    finally:
        if enc is not None:
            enc.close()
        with ph("close"):
            W.close(ok)
    stats["parts"] = W.parts
    stats["phases"] = ph.t
    if on_device:
        stats["page_kernels_ms"] = enc.ms
        stats["page_bytes_downloaded"] = enc.bytes_down
        stats["file_bytes"] = W.file_bytes
    return stats


def reads2ref(inp: str, out: str, aggregate: bool = False, min_mapq: int = 30, compression: str = "gzip",
              part_reads: int = DEFAULT_PART_READS, partition_bytes: Optional[int] = None, overwrite: bool = False,
              device: int = 0, parquet_encoder: str = "host", page_rows: Optional[int] = None,
              parquet_compressor: str = "host", region: Optional[str] = None, bai: Optional[str] = None
              ) -> Dict[str, object]:
    """`adam reads2ref`: the reads of a SAM, BAM or ADAMRecord Parquet input
    as ADAMPileup Parquet part files under `out` (which appears only when the
    job succeeds; an existing one is refused unless overwrite, and then only
    an earlier part-file directory is replaced).  min_mapq is accepted and
    ignored, as the reference never reads its -mapq.  part_reads: reads per
    part file (:data:`DEFAULT_PART_READS`); partition_bytes: SAM text per
    streamed partition (inputs.DEFAULT_PARTITION_BYTES).  parquet_encoder:
    "host" (Arrow's writer over downloaded columns) or "device" (the data
    pages built on the GPU, adam_amd/parquet_pages.py; page_rows rows per
    page, a multiple of 64); both give files that read back as the same
    table.  parquet_compressor "device": the data pages are snappy-compressed
    on the GPU before they come down (only with parquet_encoder "device" and
    compression "snappy"; a ValueError otherwise, before anything is read or
    created).  region, bai: BAM input read through its .bai index, only the reads that overlap the region (inputs.SamInput).  Returns the job's statistics."""
    if aggregate:
        raise ValueError("-aggregate is outside this build: PileupAggregator joins read names in Spark's shuffle "
                         "order, so the reference itself does not define its result")
    int(min_mapq)  # (checked to be a number, then unused: Reads2Ref.scala parses -mapq and never reads it)
    return _reads2ref(inp, out, compression, part_reads,
                      DEFAULT_PARTITION_BYTES if partition_bytes is None else partition_bytes, overwrite, device,
                      parquet_encoder=parquet_encoder, page_rows=page_rows, parquet_compressor=parquet_compressor,
                      region=region, bai=bai)


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
    ap.add_argument("-parquet_encoder", default="host", choices=("host", "device"),
                    help="where the part files' data pages are encoded (device: adam_amd/parquet_pages.py)")
    ap.add_argument("-parquet_compressor", default="host", choices=COMPRESSORS,
                    help="where the data pages are compressed (device: snappy only, with -parquet_encoder device)")
    add_region_arguments(ap)
    a = ap.parse_args(argv)
    if a.aggregate:
        ap.error("-aggregate is outside this build (PileupAggregator's result depends on Spark's shuffle order)")
    why = compressor_refusal(a.parquet_compressor, a.parquet_encoder, a.parquet_compression)
    if why:
        ap.error(why)
    try:
        a.region = region_plan(a.input, a.region, a.bai)
    except (ValueError, OSError) as e:
        ap.error(str(e))
    t0 = time.perf_counter()
    st = reads2ref(a.input, a.output, False, a.mapq, a.parquet_compression, a.part_reads, a.partition_bytes,
                   a.overwrite, parquet_encoder=a.parquet_encoder, parquet_compressor=a.parquet_compressor,
                   region=a.region, bai=a.bai)
    report(st, t0)
    return 0


if __name__ == "__main__":
    sys.exit(main())
