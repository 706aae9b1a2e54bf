"""`transform -parquet_encoder device`: the ADAMRecord part files' data pages
built on the device.

The record-level columns of a part stay where ``bqsr_sam_adam_prepare`` and
pass 2 left them (``bqsr_sam_adam_device_columns``: their device addresses, no
copy) and the page encoder (parquet_pages.py, adam_amd/csrc/parquet_pages.hip)
reads them there; only the encoded pages come down.  :func:`part_columns`
builds the 40 ``parquet_pages.Column`` of one part, in ``ADAM_FIELDS`` order:

==========================================  =====================================
the six per-read strings (``STR_COLS``)     PLAIN BYTE_ARRAY
                                            (``bqsr_parquet_pages_size_strings``);
                                            ``cigar`` too: the host path writes
                                            it through a dictionary, and a string
                                            dictionary built on the device is out
                                            of scope
the eleven booleans                         PLAIN BOOLEAN, never null
                                            (``bqsr_parquet_pages_size_bools``)
``start``, ``mateAlignmentStart``           PLAIN int64 with their validity
``referenceId``, ``mapq``,                  ``parquet_pages.small_int_column``
``mateReferenceId``, ``recordGroupId``
the 17 columns that depend only on the      DICT_INDEX over the id column
@SQ entry or the read group                 (referenceId, mateReferenceId or
                                            recordGroupId) with its validity
==========================================  =====================================

A header-derived column's dictionary page holds only the header entries that
have the value; ``remap`` sends an entry without it to -1, which makes the row
null -- the nulls ``adam_save.adam_table``'s ``lookup`` produces.  A column none
of whose entries has the value is a one-entry dictionary nothing points into:
it reads back all null.  Columns whose index streams are equal (the same id
column, the same entries present) share one ``Stream``: encoded and compressed
once.  Under gzip ``sequence`` and ``qual`` are literal-only Huffman blocks, as
``adam_save.HUFFMAN_COLS`` are on the host path.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional

import numpy as np

from . import _capi
from . import parquet_pages as PP
from ._capi import check, i64, vp
from .adam_save import (ADAM_FIELDS, BOOL_COLS, HUFFMAN_COLS, I32_COLS, I64_COLS, RG_TAGS, STR_COLS, AdamHost,
                        AdamSizes, HeaderInfo, _lib as _save_lib)

PLAIN_BYTE_ARRAY, PLAIN_BOOLEAN = 3, 4
# Rows per data page of the six string columns: 8192 reads of 100 bases are about 0.8 MB of sequence or qual, the
# size class of DEFAULT_PAGE_ROWS' 512 KB of int64 (not measured against other values).
STRING_PAGE_ROWS = 8192

_SIG = {
    "bqsr_sam_adam_device_columns": (ctypes.c_int, [vp, vp, ctypes.POINTER(AdamHost), vp]),
    "bqsr_parquet_pages_size_strings": (ctypes.c_int, [vp, vp, vp, vp, i64, i64, vp, ctypes.POINTER(PP.PagesSizes)]),
    "bqsr_parquet_pages_size_bools": (ctypes.c_int, [vp, vp, vp, i64, i64, vp, ctypes.POINTER(PP.PagesSizes)]),
}


def _lib():
    PP._lib()
    return _capi.bind(_capi.lib(), _SIG)


def encode_strings(enc: PP.Encoder, offsets, data, validity, n_rows: int, page_rows: int = STRING_PAGE_ROWS,
                   stream=None) -> PP.Stream:
    """An Arrow string column in device memory (addresses: int32 offsets
    [n_rows + 1], bytes, validity bitmap in u64 words or None) as PLAIN
    BYTE_ARRAY pages."""
    sz = PP.PagesSizes()
    check(_lib().bqsr_parquet_pages_size_strings(enc.h, offsets, data, validity, n_rows, page_rows, stream,
                                                 ctypes.byref(sz)))
    return enc.emit(sz, stream)


def encode_bools(enc: PP.Encoder, bits, validity, n_rows: int, page_rows: int = PP.DEFAULT_PAGE_ROWS,
                 stream=None) -> PP.Stream:
    """An Arrow boolean column in device memory (addresses: value bitmap and
    validity bitmap or None, u64 words) as PLAIN BOOLEAN pages."""
    sz = PP.PagesSizes()
    check(_lib().bqsr_parquet_pages_size_bools(enc.h, bits, validity, n_rows, page_rows, stream, ctypes.byref(sz)))
    return enc.emit(sz, stream)


def header_columns(hdr: HeaderInfo):
    """the 17 header-derived columns: (name, arrow type name, id column, per-entry values with None for none)"""
    sq_name = [r["SN"] for r in hdr.sq]
    sq_len, sq_url = hdr.sq_column("LN", "int"), hdr.sq_column("UR")
    out = [("referenceName", "string", "ref", sq_name), ("referenceLength", "int64", "ref", sq_len),
           ("referenceUrl", "string", "ref", sq_url), ("mateReference", "string", "mref", sq_name),
           ("mateReferenceLength", "int64", "mref", sq_len), ("mateReferenceUrl", "string", "mref", sq_url),
           ("recordGroupName", "string", "rg", hdr.rg_column("ID"))]
    out += [(name, "string", "rg", hdr.rg_column(key)) for name, key in RG_TAGS]
    out += [("recordGroupRunDateEpoch", "int64", "rg", hdr.rg_column("DT", "date")),
            ("recordGroupPredictedMedianInsertSize", "int32", "rg", hdr.rg_column("PI", "int"))]
    return out


def page_columns(enc: PP.Encoder, D: AdamHost, n: int, hdr: HeaderInfo, compression: Optional[str],
                 page_rows: Optional[int] = None, device: int = 0, stream=None) -> List[PP.Column]:
    """The 40 parquet_pages.Column of a part of n records from the device
    columns D (bqsr_sam_adam_device_columns): what adam_save.adam_table builds
    on the host, as descriptors.  page_rows: rows per page of every column
    (None: DEFAULT_PAGE_ROWS, STRING_PAGE_ROWS for the strings)."""
    import torch
    rows = PP.DEFAULT_PAGE_ROWS if page_rows is None else int(page_rows)
    string_rows = STRING_PAGE_ROWS if page_rows is None else int(page_rows)
    dev = torch.device("cuda", device)
    held = []  # the uploaded remap tables, alive until the last encode

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
        held.append(t)
        return t.data_ptr()

    cols: Dict[str, PP.Column] = {}
    gzip = compression == "gzip"
    for c, name in enumerate(STR_COLS):
        st = encode_strings(enc, D.str_offsets[c], D.str_bytes[c], D.str_valid[c], n, string_rows, stream)
        cols[name] = PP.Column(name, "string", st, huffman=gzip and name in HUFFMAN_COLS)
    for c, name in enumerate(BOOL_COLS):
        cols[name] = PP.Column(name, "bool", encode_bools(enc, D.bools[c], None, n, rows, stream))
    for c, name in enumerate(I64_COLS):
        d = PP.ParquetColumn(kind=PP.PLAIN_INT64, src_width=8, src=D.i64[c], src_n=n, validity=D.int_valid[4 + c])
        cols[name] = PP.Column(name, "int64", enc.encode(d, n, rows, stream))
    for c, name in enumerate(I32_COLS):
        d = PP.ParquetColumn(kind=PP.PLAIN_INT32, src_width=4, src=D.i32[c], src_n=n, validity=D.int_valid[c])
        cols[name] = PP.small_int_column(enc, name, d, n, rows, stream)
    # by index: the id column mapped through the field's entry -> dictionary index table, in which an entry
    # without the value is -1; equal index streams are encoded once
    ids = {"ref": 0, "mref": 2, "rg": 3}  # (I32_COLS)
    streams: Dict[tuple, PP.Stream] = {}
    for name, kind, which, values in header_columns(hdr):
        has = np.asarray([v is not None for v in values], bool)
        remap = np.where(has, np.cumsum(has) - 1, -1).astype(np.int32) if len(values) else np.full(1, -1, np.int32)
        key = (which, remap.tobytes())
        if key not in streams:
            c = ids[which]
            d = PP.ParquetColumn(kind=PP.DICT_INDEX, src_width=4, src=D.i32[c], src_n=n, remap=up(remap),
                                 remap_n=len(remap), bit_width=PP.bit_width(int(has.sum())),
                                 validity=D.int_valid[c])
            streams[key] = enc.encode(d, n, rows, stream)
        entries = [v for v in values if v is not None] or ["" if kind == "string" else 0]
        dic = PP.plain_strings(entries) if kind == "string" else PP.plain_ints(entries, kind)
        cols[name] = PP.Column(name, kind, streams[key], dic)
    del held
    return [cols[name] for name, _ in ADAM_FIELDS]


def part_columns(sam, enc: PP.Encoder, r0: int, n: int, hdr: HeaderInfo, compression: Optional[str],
                 page_rows: Optional[int] = None, device: int = 0, stream=None) -> List[PP.Column]:
    """the columns of records [r0, r0 + n) of a parse (sam.SamText), its pages
    encoded on the device, from its current text and quals (adam_save.set_quals)"""
    L = _lib()
    sz = AdamSizes()
    check(_save_lib().bqsr_sam_adam_prepare(sam.ctx.handle, sam.h, r0, n, stream, ctypes.byref(sz)))
    D = AdamHost()
    check(L.bqsr_sam_adam_device_columns(sam.ctx.handle, sam.h, ctypes.byref(D), stream))
    return page_columns(enc, D, n, hdr, compression, page_rows, device, stream)
