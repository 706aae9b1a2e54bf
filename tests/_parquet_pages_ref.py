"""The three page forms of bqsr_parquet_pages_* restated in numpy from the
Parquet format text (Encodings.md: PLAIN, the RLE / bit-packed hybrid; data
page V1: u32-length-prefixed definition levels, then the values), with the
block rule of include/adam_sam.h.  Independent of the kernels: plain Python
loops over pages and blocks."""
import struct

import numpy as np

PLAIN_INT32, PLAIN_INT64, DICT_INDEX = 0, 1, 2


def varint(n: int) -> bytes:
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        out.append(b | (0x80 if n else 0))
        if not n:
            return bytes(out)


def bit_packed_run(vals, w: int) -> bytes:
    """<varint groups << 1 | 1> <groups * 8 values, w bits each, LSB first, zero-padded>"""
    v = np.asarray(vals, np.uint64)
    groups = (len(v) + 7) // 8
    v = np.concatenate([v, np.zeros(groups * 8 - len(v), np.uint64)])
    bits = ((v[:, None] >> np.arange(w, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8).ravel()
    return varint((groups << 1) | 1) + np.packbits(bits, bitorder="little").tobytes()


def rle_run(value: int, count: int, w: int) -> bytes:
    return varint(count << 1) + int(value).to_bytes((w + 7) // 8, "little")


def levels(valid) -> bytes:
    """definition levels of max level 1: the bitmap as ONE bit-packed run, behind its u32 length"""
    run = bit_packed_run(np.asarray(valid, bool).astype(np.uint64), 1)
    return struct.pack("<I", len(run)) + run


def indices(vals, w: int) -> bytes:
    """<bit width> then blocks of 64: a full block of equal values is an RLE run, any other a bit-packed run"""
    out = bytes([w])
    vals = np.asarray(vals, np.uint64) & np.uint64((1 << w) - 1)
    for p in range(0, len(vals), 64):
        blk = vals[p:p + 64]
        if len(blk) == 64 and (blk == blk[0]).all():
            out += rle_run(int(blk[0]), 64, w)
        else:
            out += bit_packed_run(blk, w)
    return out


def row_values(n_rows, src, gather=None, remap=None, base=0, validity=None):
    """(values int64, valid bool) of a bqsr_parquet_column's rows"""
    src = np.asarray(src).astype(np.int64)
    valid = np.ones(n_rows, bool) if validity is None else np.asarray(validity, bool)[:n_rows].copy()
    i = np.arange(n_rows) if gather is None else np.asarray(gather, np.int64)[:n_rows]
    valid &= (i >= 0) & (i < len(src))
    v = src[np.where(valid, i, 0)] if len(src) else np.zeros(n_rows, np.int64)
    if remap is not None:
        remap = np.asarray(remap, np.int64)
        valid &= (v >= 0) & (v < len(remap))
        v = remap[np.where(valid, v, 0)]
        valid &= v >= 0
    return np.where(valid, v - base, 0), valid


def column_pages(kind, values, valid, page_rows, w=0):
    """(bodies, pages [n_pages, 4]: offset, bytes, rows, non-nulls) of a column chunk"""
    values, valid = np.asarray(values, np.int64), np.asarray(valid, bool)
    bodies, pages = b"", []
    for r in range(0, len(values), page_rows):
        ok = valid[r:r + page_rows]
        v = values[r:r + page_rows][ok]
        if kind == DICT_INDEX:
            body = levels(ok) + indices(v, w)
        else:
            body = levels(ok) + v.astype("<i4" if kind == PLAIN_INT32 else "<i8").tobytes()
        pages.append((len(bodies), len(body), len(ok), int(ok.sum())))
        bodies += body
    return bodies, np.asarray(pages, np.int64).reshape(-1, 4)


def bitmap_words(valid) -> np.ndarray:
    """an Arrow validity bitmap in u64 words"""
    valid = np.asarray(valid, bool)
    b = np.packbits(valid, bitorder="little")
    out = np.zeros(max(1, (len(valid) + 63) // 64) * 8, np.uint8)
    out[:len(b)] = b
    return out.view(np.uint64)
