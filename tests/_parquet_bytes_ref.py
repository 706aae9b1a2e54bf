"""The PLAIN BYTE_ARRAY and PLAIN BOOLEAN page bodies of
bqsr_parquet_pages_size_strings / _bools restated in numpy from the Parquet
format text (Encodings.md, PLAIN: a BYTE_ARRAY is its 4-byte little-endian
length and its bytes; a BOOLEAN is one bit, LSB first), behind the definition
levels of tests/_parquet_pages_ref.py.  Independent of the kernels: plain
Python loops over pages and rows."""
import struct

import numpy as np

from _parquet_pages_ref import levels


def column_pages_strings(offsets, data, valid, page_rows):
    """(bodies, pages [n_pages, 4]: offset, bytes, rows, non-nulls) of an
    Arrow string column: int32 offsets [n + 1], its bytes, valid bool [n]"""
    offsets = np.asarray(offsets, np.int64)
    data = data if isinstance(data, bytes) else bytes(np.asarray(data, np.uint8))
    valid = np.asarray(valid, bool)
    bodies, pages = b"", []
    for r in range(0, len(valid), page_rows):
        ok = valid[r:r + page_rows]
        body = levels(ok)
        for i in np.flatnonzero(ok):
            a, b = int(offsets[r + i]), int(offsets[r + i + 1])
            body += struct.pack("<I", b - a) + data[a:b]
        pages.append((len(bodies), len(body), len(ok), int(ok.sum())))
        bodies += body
    return bodies, np.asarray(pages, np.int64).reshape(-1, 4)


def column_pages_bools(bits, valid, page_rows):
    """the same of a boolean column: bits bool [n] (its values), valid bool [n]"""
    bits, valid = np.asarray(bits, bool), np.asarray(valid, bool)
    bodies, pages = b"", []
    for r in range(0, len(valid), page_rows):
        ok = valid[r:r + page_rows]
        body = levels(ok) + np.packbits(bits[r:r + page_rows][ok], bitorder="little").tobytes()
        pages.append((len(bodies), len(body), len(ok), int(ok.sum())))
        bodies += body
    return bodies, np.asarray(pages, np.int64).reshape(-1, 4)


def arrow_strings(values):
    """(offsets int32 [n + 1], bytes uint8, valid bool [n]) of a list of bytes objects, None for null"""
    off = np.zeros(len(values) + 1, np.int32)
    off[1:] = np.cumsum([0 if v is None else len(v) for v in values])
    data = np.frombuffer(b"".join(v or b"" for v in values), np.uint8).copy()
    return off, data, np.asarray([v is not None for v in values], bool)
