"""Parquet part files whose data pages were built on the device.

The device (include/adam_sam.h ``bqsr_parquet_pages_*``, adam_amd/csrc/
parquet_pages.hip) turns one column at a time, read from device memory, into
V1 data page BODIES: definition levels as the validity bitmap in one
bit-packed run, then PLAIN int32 / int64 values, dictionary indices in the
RLE / bit-packed hybrid under the header's block rule, or (from the size
calls adam_pages.py binds, for ``transform``) PLAIN BYTE_ARRAY / BOOLEAN
values.  This module is
the host's share: :class:`Encoder` drives those calls and brings a chunk's
bodies and page table back in one copy each; :class:`PagesWriter` -- an
:class:`adam_save.AdamWriter`, so with its part-file, ``.partial``,
``_SUCCESS`` and overwrite rules -- adds dictionary pages, Thrift compact page
headers, the codec (gzip through ``bqsr_gzip_bytes`` at level 6, snappy
through ``pyarrow.compress``, or none) on the writer's thread pool, and the
footer.

``Encoder(ctx, compressor="device")`` (``-parquet_compressor device``, snappy
only) compresses the data pages before they come down
(``bqsr_parquet_pages_compress`` / ``_fetch``, adam_amd/csrc/snappy_pages.hip:
every 64 KiB block of a page by one workgroup, in the raw snappy format
include/adam_sam.h declares): a :class:`Stream` then carries the compressed
pages and their offsets, the raw bodies never leave the device, and
:func:`assemble` writes them as they are.  Dictionary pages stay with
``pyarrow.compress``.  :func:`snappy_pages` and :func:`snappy_pages_host` are
the codec alone, on the device and as the same routine compiled for the host.

The files hold only what parquet-format 1.0 defines, so that parquet-mr of the
reference's vintage reads them: V1 data pages, RLE levels, PLAIN and
PLAIN_DICTIONARY.  (The Arrow writer of the host path declares
RLE_DICTIONARY, a format-2 name for the same bytes; these files declare what
Arrow's own ``version="1.0"`` writer declares: ``PLAIN_DICTIONARY, RLE`` for a
dictionary column, ``RLE, PLAIN`` for a plain one.)  The footer's schema is the
host path's: the same names, physical types, UTF8 annotation and OPTIONAL
repetition, and no ``ARROW:schema`` key.  Statistics: ``null_count`` per page
and per column chunk, from the device's popcounts; min / max are left out (no
reader of these files filters on them, and they would need a reduction per
column and, for strings, a pass over the dictionary).

Out of scope here: a string dictionary built on the device (a dictionary
page's entries come from the host), gzip pages and dictionary pages compressed
on the device, and the writers of ``transform_parquet`` and
``aggregate_pileups``.
"""
from __future__ import annotations

import ctypes
import os
import struct
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _capi
from ._capi import check, dblp, i64, i64p, vp
from .adam_save import AdamWriter, _lib as _save_lib, _pinned

PLAIN_INT32, PLAIN_INT64, DICT_INDEX = 0, 1, 2
# rows per data page: 64 Ki rows are 512 KB of PLAIN int64 and a few KB of narrow indices
DEFAULT_PAGE_ROWS = 1 << 16
# a dense int range [min, max] becomes a dictionary while it has at most this many entries
MAX_DENSE_RANGE = 65536


class ParquetColumn(ctypes.Structure):
    """bqsr_parquet_column"""
    _fields_ = [("kind", ctypes.c_int32), ("src_width", ctypes.c_int32), ("src", ctypes.c_void_p),
                ("src_n", ctypes.c_int64), ("gather", ctypes.c_void_p), ("remap", ctypes.c_void_p),
                ("remap_n", ctypes.c_int32), ("bit_width", ctypes.c_int32), ("base", ctypes.c_int64),
                ("validity", ctypes.c_void_p)]


class ParquetPage(ctypes.Structure):
    """bqsr_parquet_page"""
    _fields_ = [("offset", ctypes.c_int64), ("bytes", ctypes.c_int64), ("rows", ctypes.c_int64),
                ("non_nulls", ctypes.c_int64)]


class PagesSizes(ctypes.Structure):
    """bqsr_parquet_pages_sizes"""
    _fields_ = [("n_pages", ctypes.c_int64), ("body_bytes", ctypes.c_int64)]


KERNELS = ("size", "emit")
# the stages a device compressor adds to Encoder.ms
CODEC_KERNELS = ("snappy", "pack")
COMPRESSORS = ("host", "device")
CODEC_SNAPPY = 1  # BQSR_PARQUET_CODEC_SNAPPY
COMPRESSOR_CHOICE = "-parquet_compressor must be one of %s" % ", ".join(COMPRESSORS)
COMPRESSOR_NEEDS_ENCODER = ("-parquet_compressor device compresses the pages -parquet_encoder device builds: it "
                            "cannot be combined with -parquet_encoder host")
COMPRESSOR_NEEDS_SNAPPY = ("-parquet_compressor device has one codec: it needs -parquet_compression snappy (gzip "
                           "and none keep -parquet_compressor host)")


def compressor_refusal(compressor: str, encoder: str, compression: Optional[str]) -> Optional[str]:
    """why -parquet_compressor `compressor` cannot serve a job with this
    -parquet_encoder and -parquet_compression (None: it can)"""
    if compressor not in COMPRESSORS:
        return COMPRESSOR_CHOICE
    if compressor == "device" and encoder != "device":
        return COMPRESSOR_NEEDS_ENCODER
    if compressor == "device" and compression != "snappy":
        return COMPRESSOR_NEEDS_SNAPPY
    return None


_SIG = {
    "bqsr_parquet_pages_create": (ctypes.c_int, [vp, ctypes.POINTER(vp)]),
    "bqsr_parquet_pages_destroy": (None, [vp]),
    "bqsr_parquet_pages_size": (ctypes.c_int, [vp, ctypes.POINTER(ParquetColumn), i64, i64, vp,
                                               ctypes.POINTER(PagesSizes)]),
    "bqsr_parquet_pages_emit": (ctypes.c_int, [vp, vp, vp, vp]),
    "bqsr_parquet_pages_minmax": (ctypes.c_int, [vp, ctypes.POINTER(ParquetColumn), i64, vp, i64p, i64p, i64p]),
    "bqsr_parquet_pages_kernel_times": (ctypes.c_int, [dblp, dblp]),
}
# the snappy codec (adam_amd/csrc/snappy_pages.hip)
_CODEC_SIG = {
    "bqsr_snappy_pages": (ctypes.c_int, [vp, vp, i64p, i64, vp, vp, i64, i64p]),
    "bqsr_snappy_pages_host": (ctypes.c_int, [vp, i64p, i64, vp, i64, i64p]),
    "bqsr_parquet_pages_compress": (ctypes.c_int, [vp, ctypes.c_int32, vp, i64p]),
    "bqsr_parquet_pages_fetch": (ctypes.c_int, [vp, vp, vp, i64p, vp]),
    "bqsr_parquet_pages_compress_times": (ctypes.c_int, [dblp, dblp]),
}


def _lib():
    return _capi.bind(_capi.bind(_capi.lib(), _SIG), _CODEC_SIG)


def kernel_times():
    """(size ms, emit ms) of this thread's last size / emit calls, by device
    events (measurement only)"""
    return tuple(_capi.stage_times(_lib().bqsr_parquet_pages_kernel_times, KERNELS).values())


def compress_times():
    """(snappy ms, pack ms) of this thread's last device compress call, by
    device events (measurement only)"""
    return tuple(_capi.stage_times(_lib().bqsr_parquet_pages_compress_times, CODEC_KERNELS).values())


def _snappy_call(call, data, offsets):
    """pages of `data` cut at `offsets` [n_pages + 1] through one of the two
    codec entry points: (the packed pages as a uint8 array, int64 offsets
    [n_pages + 1]); a first call with the usual bound, a second with the size
    the first reports when that was short"""
    a = np.ascontiguousarray(np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else data)
    off = np.ascontiguousarray(offsets, np.int64)
    n_pages = len(off) - 1
    if n_pages < 0:
        raise ValueError("offsets has n_pages + 1 entries")
    out_off = np.zeros(n_pages + 1, np.int64)
    cap = int(off[-1] - off[0]) // 32 * 33 + 16 * n_pages + 64 if n_pages else 0
    while True:
        out = np.empty(cap, np.uint8)
        rc = call(a.ctypes.data if len(a) else None, off.ctypes.data_as(i64p), n_pages,
                  out.ctypes.data if cap else None, cap, out_off.ctypes.data_as(i64p))
        if rc == _capi.INVALID_ARG and n_pages and int(out_off[-1]) > cap:
            cap = int(out_off[-1])
            continue
        check(rc)
        return out[:int(out_off[-1])], out_off


def snappy_pages(data, offsets, ctx=None, stream=None):
    """The pages data[offsets[i]:offsets[i + 1]] compressed on the device
    (``bqsr_snappy_pages``): (packed uint8 array, int64 offsets [n_pages +
    1]).  Every page is a raw snappy stream any snappy decoder reads."""
    from . import bqsr
    L, ctx = _lib(), ctx or bqsr.Context.get(0)
    return _snappy_call(lambda a, off, n, out, cap, oo: L.bqsr_snappy_pages(ctx.handle, a, off, n, stream, out, cap, oo),
                        data, offsets)


def snappy_pages_host(data, offsets):
    """:func:`snappy_pages` by the block routine compiled for the host
    (``bqsr_snappy_pages_host``): the same bytes, no device"""
    return _snappy_call(_lib().bqsr_snappy_pages_host, data, offsets)


def bit_width(n_entries: int) -> int:
    """the index width of a dictionary of n_entries (at least 1)"""
    return max(1, (max(1, int(n_entries)) - 1).bit_length())


class Stream:
    """One encoded column chunk: `bodies`, the concatenated page bodies (a
    uint8 array), and `pages`, int64 [n_pages, 4]: body offset, body bytes,
    rows, non-nulls.  Columns whose index streams are equal share one.  From a
    device compressor: `comp`, the pages already under `codec`, page i being
    comp[comp_off[i]:comp_off[i + 1]]; `bodies` is None then (the raw bytes
    stayed on the device) and `pages` still holds the RAW sizes."""

    def __init__(self, bodies: Optional[np.ndarray], pages: np.ndarray, comp: Optional[np.ndarray] = None,
                 comp_off: Optional[np.ndarray] = None, codec: Optional[str] = None):
        self.bodies = bodies
        self.pages = np.asarray(pages, np.int64).reshape(-1, 4)
        self.comp = comp
        self.comp_off = None if comp is None else np.asarray(comp_off, np.int64)
        self.codec = codec if comp is not None else None
        assert comp is None or len(self.comp_off) == len(self.pages) + 1


class Column:
    """A column of a part file: its Arrow type name ("string", "int32",
    "int64", "bool"), its stream, and for a dictionary column the
    PLAIN-encoded dictionary page body with its entry count (None: PLAIN data
    pages).  huffman: under gzip its data pages are literal-only Huffman
    blocks (``bqsr_gzip_bytes(huffman=1)``: per-base strings, whose letter
    frequencies are their redundancy), as adam_save.HUFFMAN_COLS are on the
    host path."""

    def __init__(self, name: str, kind: str, stream: Stream, dictionary: Optional[Tuple[object, int]] = None,
                 huffman: bool = False):
        self.name = name
        self.kind = kind
        self.stream = stream
        self.dictionary = dictionary
        self.huffman = bool(huffman)


class Encoder:
    """The device encoder of one context: `encode` a column chunk into a
    :class:`Stream`, `minmax` for a dense-range dictionary.  Sums the kernels'
    device-event times (`ms`) and the bytes downloaded (`bytes_down`).
    compressor "device": the streams come down snappy-compressed (see
    :class:`Stream`), and `ms` has the codec's two stages too."""

    def __init__(self, ctx, compressor: str = "host"):
        if compressor not in COMPRESSORS:
            raise ValueError("compressor must be one of %s" % ", ".join(COMPRESSORS))
        self.ctx = ctx
        self.compressor = compressor
        self.h = vp()
        check(_lib().bqsr_parquet_pages_create(ctx.handle, ctypes.byref(self.h)))
        self.ms = dict.fromkeys(KERNELS + (CODEC_KERNELS if compressor == "device" else ()), 0.0)
        self.bytes_down = 0

    def close(self):
        if self.h:
            _lib().bqsr_parquet_pages_destroy(self.h)
            self.h = vp()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def encode(self, col: ParquetColumn, n_rows: int, page_rows: int = DEFAULT_PAGE_ROWS, stream=None) -> Stream:
        L = _lib()
        sz = PagesSizes()
        check(L.bqsr_parquet_pages_size(self.h, ctypes.byref(col), n_rows, page_rows, stream, ctypes.byref(sz)))
        return self.emit(sz, stream)

    def emit(self, sz: PagesSizes, stream=None) -> Stream:
        """the emit call after a size call -- or, with the device compressor,
        compress and fetch -- and its share of `ms` and `bytes_down`"""
        L = _lib()
        pages = np.zeros((sz.n_pages, 4), np.int64)
        if self.compressor == "device":
            n = ctypes.c_int64()
            check(L.bqsr_parquet_pages_compress(self.h, CODEC_SNAPPY, stream, ctypes.byref(n)))
            comp = _pinned(n.value)[:n.value]
            comp_off = np.zeros(sz.n_pages + 1, np.int64)
            check(L.bqsr_parquet_pages_fetch(self.h, comp.ctypes.data if n.value else None,
                                             pages.ctypes.data if sz.n_pages else None,
                                             comp_off.ctypes.data_as(i64p), stream))
            for k, v in zip(CODEC_KERNELS, compress_times()):
                self.ms[k] += v
            st = Stream(None, pages, comp, comp_off, "snappy")
            # what came down: the packed pages, the page table, and the offsets of the size table's items (a
            # page's varint and each of its 64 KiB blocks), from which the library cuts comp_off
            items = sz.n_pages + int(((pages[:, 1] + 65535) // 65536).sum())
            self.bytes_down += n.value + pages.nbytes + 8 * (items + 1) if sz.n_pages else 0
        else:
            bodies = _pinned(sz.body_bytes)[:sz.body_bytes]
            check(L.bqsr_parquet_pages_emit(self.h, bodies.ctypes.data if sz.body_bytes else None,
                                            pages.ctypes.data if sz.n_pages else None, stream))
            st = Stream(bodies, pages)
            self.bytes_down += sz.body_bytes + pages.nbytes
        for k, v in zip(KERNELS, kernel_times()):
            self.ms[k] += v
        return st

    def minmax(self, col: ParquetColumn, n_rows: int, stream=None) -> Tuple[int, int, int]:
        """(min, max, non-null count) of the column's values (min > max: none)"""
        lo, hi, nn = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        check(_lib().bqsr_parquet_pages_minmax(self.h, ctypes.byref(col), n_rows, stream, ctypes.byref(lo),
                                               ctypes.byref(hi), ctypes.byref(nn)))
        return lo.value, hi.value, nn.value


def small_int_column(enc: Encoder, name: str, plain: ParquetColumn, n_rows: int,
                     page_rows: int = DEFAULT_PAGE_ROWS, stream=None) -> Column:
    """An int32 column given as its PLAIN descriptor: after a min / max
    reduction over the part, a dictionary column over the dense range [min,
    max] with index = value - min when the range has at most MAX_DENSE_RANGE
    entries (entries no row uses are legal), else the PLAIN column."""
    lo, hi, nn = enc.minmax(plain, n_rows, stream)
    if nn == 0:
        lo = hi = 0
    if hi - lo + 1 > MAX_DENSE_RANGE:
        return Column(name, "int32", enc.encode(plain, n_rows, page_rows, stream))
    d = ParquetColumn.from_buffer_copy(plain)
    d.kind, d.base, d.bit_width = DICT_INDEX, lo, bit_width(hi - lo + 1)
    return Column(name, "int32", enc.encode(d, n_rows, page_rows, stream),
                  plain_ints(np.arange(lo, hi + 1), "int32"))


# ---- dictionary pages (PLAIN) ----

def plain_ints(values, kind: str) -> Tuple[bytes, int]:
    a = np.asarray(values, "<i4" if kind == "int32" else "<i8")
    return a.tobytes(), len(a)


def plain_strings(values: Sequence[str]) -> Tuple[bytes, int]:
    raw = [v.encode("utf-8") for v in values]
    return b"".join(struct.pack("<i", len(r)) + r for r in raw), len(raw)


def plain_string_array(arr) -> Tuple[np.ndarray, int]:
    """a pyarrow StringArray (no nulls) as a PLAIN dictionary page body, without a step per string"""
    n = len(arr)
    bufs = arr.buffers()
    off = np.frombuffer(bufs[1], np.int32, n + 1, arr.offset * 4).astype(np.int64)
    data = np.frombuffer(bufs[2], np.uint8) if bufs[2] is not None else np.zeros(0, np.uint8)
    data = data[off[0]:off[n]]
    lens = np.diff(off)
    out = np.empty(len(data) + 4 * n, np.uint8)
    at = off[:-1] - off[0] + 4 * np.arange(n, dtype=np.int64)  # each string's length prefix
    out[at[:, None] + np.arange(4)] = lens.astype("<i4").view(np.uint8).reshape(n, 4)
    out[np.arange(len(data), dtype=np.int64) + 4 * np.repeat(np.arange(1, n + 1, dtype=np.int64), lens)] = data
    return out, n


# ---- Thrift compact protocol (what parquet.thrift's structures need) ----

def _varint(n: int) -> bytes:
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        if n:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _zigzag(n: int) -> bytes:
    return _varint((n << 1) ^ (n >> 63))


class _Struct:
    I32, I64, BINARY, LIST, STRUCT = 5, 6, 8, 9, 12

    def __init__(self):
        self.b = bytearray()
        self.last = 0

    def _field(self, fid: int, typ: int, payload: bytes):
        d = fid - self.last
        self.b += bytes([(d << 4) | typ]) if 0 < d < 16 else bytes([typ]) + _zigzag(fid)
        self.b += payload
        self.last = fid
        return self

    def i32(self, fid, v):
        return self._field(fid, self.I32, _zigzag(v))

    def i64(self, fid, v):
        return self._field(fid, self.I64, _zigzag(v))

    def binary(self, fid, v: bytes):
        return self._field(fid, self.BINARY, _varint(len(v)) + v)

    def struct(self, fid, sub: "_Struct"):
        return self._field(fid, self.STRUCT, sub.end())

    def list(self, fid, typ, items: Sequence[bytes]):
        n = len(items)
        head = bytes([(n << 4) | typ]) if n < 15 else bytes([0xF0 | typ]) + _varint(n)
        return self._field(fid, self.LIST, head + b"".join(items))

    def end(self) -> bytes:
        return bytes(self.b) + b"\0"


# parquet.thrift's enums
_TYPE = {"bool": 0, "int32": 1, "int64": 2, "string": 6}  # BOOLEAN, INT32, INT64, BYTE_ARRAY
_CODEC = {None: 0, "snappy": 1, "gzip": 2}
_ENC_PLAIN, _ENC_PLAIN_DICTIONARY, _ENC_RLE = 0, 2, 3
_DATA_PAGE, _DICTIONARY_PAGE = 0, 2
_OPTIONAL, _REQUIRED = 1, 0
CREATED_BY = b"adam_amd device pages"


def _data_page_header(raw: int, comp: int, rows: int, non_nulls: int, dictionary: bool) -> bytes:
    stats = _Struct().i64(3, rows - non_nulls)
    h = _Struct().i32(1, rows).i32(2, _ENC_PLAIN_DICTIONARY if dictionary else _ENC_PLAIN).i32(3, _ENC_RLE)
    h.i32(4, _ENC_RLE).struct(5, stats)
    return _Struct().i32(1, _DATA_PAGE).i32(2, raw).i32(3, comp).struct(5, h).end()


def _dictionary_page_header(raw: int, comp: int, count: int) -> bytes:
    h = _Struct().i32(1, count).i32(2, _ENC_PLAIN_DICTIONARY)
    return _Struct().i32(1, _DICTIONARY_PAGE).i32(2, raw).i32(3, comp).struct(7, h).end()


def _schema_elements(fields: Sequence[Tuple[str, str]]) -> List[bytes]:
    out = [_Struct().i32(3, _REQUIRED).binary(4, b"schema").i32(5, len(fields)).end()]
    for name, kind in fields:
        e = _Struct().i32(1, _TYPE[kind]).i32(3, _OPTIONAL).binary(4, name.encode())
        if kind == "string":  # converted_type UTF8, and the logical type STRING that later readers look for
            e.i32(6, 0).struct(10, _Struct().struct(1, _Struct()))
        out.append(e.end())
    return out


def gzip_bytes(buf: np.ndarray, level: int = 6, huffman: bool = False) -> bytes:
    """one gzip member of `buf` through the library (libdeflate / zlib at
    `level`; huffman: one literal-only Huffman block)"""
    L = _save_lib()
    n = ctypes.c_int64()
    cap = len(buf) + len(buf) // 8 + 64
    while True:
        out = np.empty(cap, np.uint8)
        check(L.bqsr_gzip_bytes(buf.ctypes.data if len(buf) else None, len(buf), int(huffman), level, out.ctypes.data,
                                cap, ctypes.byref(n)))
        if n.value <= cap:
            return out[:n.value].tobytes()
        cap = n.value


def compress(codec: Optional[str], buf, huffman: bool = False) -> object:
    """a page body under the codec (None: as it is); huffman: see :class:`Column` (gzip only)"""
    if codec is None:
        return buf
    a = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf
    if codec == "gzip":
        return gzip_bytes(np.ascontiguousarray(a), huffman=huffman)
    import pyarrow as pa
    return pa.compress(pa.py_buffer(a), codec=codec, asbytes=True)


# page bodies compressed per task: enough work to amortise a task, small enough to spread a wide column
_TASK_BYTES = 4 << 20


def assemble(path: str, fields: Sequence[Tuple[str, str]], columns: Sequence[Column], n_rows: int,
             codec: Optional[str], pool: Optional[ThreadPoolExecutor] = None) -> int:
    """Write one Parquet file of `columns` (in `fields`' order; none: a file
    of the schema alone) with one row group; the page bodies are compressed on
    `pool`.  Returns the file's size."""
    assert [c.name for c in columns] == [n for n, _ in fields] or not columns
    run = (lambda f, *a: pool.submit(f, *a)) if pool else (lambda f, *a: _Done(f(*a)))

    def pages_of(st: Stream, a: int, b: int, huffman: bool):
        if st.comp is not None:  # compressed on the device: as they are
            if st.codec != codec:
                raise ValueError("a stream compressed as %s in a file of codec %s" % (st.codec, codec))
            return [st.comp[st.comp_off[p]:st.comp_off[p + 1]] for p in range(a, b)]
        return [compress(codec, st.bodies[o:o + nb], huffman) for o, nb in st.pages[a:b, :2]]

    # every distinct stream once (per form), cut into tasks of whole pages
    jobs: Dict[Tuple[int, bool], list] = {}
    for c in columns:
        st = c.stream
        if (id(st), c.huffman) in jobs:
            continue
        tasks, a, acc = [], 0, 0
        for p in range(len(st.pages)):
            acc += int(st.pages[p, 1])
            if acc >= _TASK_BYTES or p + 1 == len(st.pages):
                tasks.append(run(pages_of, st, a, p + 1, c.huffman))
                a, acc = p + 1, 0
        jobs[(id(st), c.huffman)] = tasks
    dicts = [run(compress, codec, c.dictionary[0]) if c.dictionary else None for c in columns]
    with open(path, "wb") as fh:
        fh.write(b"PAR1")
        pos = 4
        chunks = []
        total = 0
        for c, dj in zip(columns, dicts):
            start, raw_size, nulls = pos, 0, 0
            dict_off = None
            if c.dictionary:
                body, count = c.dictionary
                comp = dj.result()
                head = _dictionary_page_header(len(body), len(comp), count)
                dict_off = pos
                fh.write(head)
                fh.write(comp)
                pos += len(head) + len(comp)
                raw_size += len(head) + len(body)
            data_off = pos
            done = [x for t in jobs[(id(c.stream), c.huffman)] for x in t.result()]
            for (o, nb, rows, nn), comp in zip(c.stream.pages.tolist(), done):
                head = _data_page_header(nb, len(comp), rows, nn, c.dictionary is not None)
                fh.write(head)
                fh.write(comp)
                pos += len(head) + len(comp)
                raw_size += len(head) + nb
                nulls += rows - nn
            enc = [_ENC_PLAIN_DICTIONARY, _ENC_RLE] if c.dictionary else [_ENC_RLE, _ENC_PLAIN]
            md = _Struct().i32(1, _TYPE[c.kind]).list(2, _Struct.I32, [_zigzag(e) for e in enc])
            md.list(3, _Struct.BINARY, [_varint(len(c.name.encode())) + c.name.encode()]).i32(4, _CODEC[codec])
            md.i64(5, n_rows).i64(6, raw_size).i64(7, pos - start).i64(9, data_off)
            if dict_off is not None:
                md.i64(11, dict_off)
            md.struct(12, _Struct().i64(3, nulls))
            chunks.append(_Struct().i64(2, start).struct(3, md).end())
            total += pos - start
        groups = [_Struct().list(1, _Struct.STRUCT, chunks).i64(2, total).i64(3, n_rows).end()] if columns else []
        footer = _Struct().i32(1, 1).list(2, _Struct.STRUCT, _schema_elements(fields)).i64(3, n_rows)
        footer = footer.list(4, _Struct.STRUCT, groups).binary(6, CREATED_BY).end()
        fh.write(footer)
        fh.write(struct.pack("<I", len(footer)))
        fh.write(b"PAR1")
        return pos + len(footer) + 8


class _Done:
    def __init__(self, v):
        self.v = v

    def result(self):
        return self.v


class PagesWriter(AdamWriter):
    """AdamWriter's directory of part files (``OUT.partial`` renamed to
    ``OUT`` on ``close``, the same overwrite rules), each part assembled from
    device-built page bodies: the pool compresses pages, one more thread per
    pending part puts its file together."""

    def __init__(self, path: str, fields: Sequence[Tuple[str, str]], compression: str = "gzip",
                 threads: Optional[int] = None, overwrite: bool = False, max_pending: int = 2):
        super().__init__(path, compression, threads=threads, overwrite=overwrite, max_pending=max_pending)
        self.fields = list(fields)
        self.filer = ThreadPoolExecutor(max_workers=self.max_pending + 1)
        self.file_bytes = 0

    def _write_part(self, columns, n_rows, name):
        return assemble(os.path.join(self.tmp, name), self.fields, columns, n_rows, self.compression, self.pool)

    def add(self, columns: Sequence[Column], n_rows: int):
        """one part file of `columns` (none: the schema alone)"""
        name = "part-r-%05d.parquet" % self.parts
        self.parts += 1
        self.rows += n_rows
        self.futures.append(self.filer.submit(self._write_part, list(columns), n_rows, name))
        while len(self.futures) > self.max_pending:
            self.file_bytes += self.futures.pop(0).result()

    def close(self, ok: bool = True):
        rest = list(self.futures)
        try:
            super().close(ok)
        finally:
            self.filer.shutdown(wait=True)
        if ok:
            self.file_bytes += sum(f.result() for f in rest)
