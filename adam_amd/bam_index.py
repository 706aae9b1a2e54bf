"""Index an existing BAM, and read a region of a BAM through its .bai index.

    python -m adam_amd.bam_index IN.bam [-output FILE] [-overwrite] [-piece_bytes N]

writes IN.bam.bai for a BAM any tool wrote (SAM spec §5.2; the rules are in
include/adam_sam.h at bqsr_bam_index_create): the file is read in windows of
whole BGZF members (bqsr_bam_reader_*, bam_windows.hip), every window inflated
on the device, its records found there and a row each left in the device index
(bam_index.hip) that `transform -bam_index` builds too.  Device memory is
bounded by the window (`piece_bytes` of inflated stream), not by the file.

``BaiIndex`` reads a .bai trusting only the spec, ``parse_region`` the
``-region`` syntax, and ``region_text`` parses the records of one region: only
the members the index names are read, inflated and walked; a device kernel
keeps the records that overlap the region and compacts them into one buffer,
which takes bqsr_bam_parse's path to an ordinary ``SamText``
(``inputs.SamInput(region=...)``).
"""
from __future__ import annotations

import argparse
import ctypes
import mmap
import os
import struct
import sys
import time
import zlib
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _capi
from ._capi import check, i32, i64, i64p, pp, vp

DEFAULT_PIECE_BYTES = 1 << 30  # of inflated stream per window: bgzf_inflate_runs' run size
MAX_END = 1 << 29              # BAI's limit
PSEUDO_BIN = 37450


class BamWindow(ctypes.Structure):
    _fields_ = [("n_records", i64), ("member_begin", i64), ("member_end", i64), ("next_pos", i64),
                ("device", i32), ("done", i32)]


class BamReaderStats(ctypes.Structure):
    _fields_ = [(n, i64) for n in ("members_total", "stream_bytes", "n_ref", "body", "members_read", "windows_device",
                                   "windows_host", "records_seen", "records_kept", "members_host")] + [("filter_ms", ctypes.c_double)]


_SIG = {
    "bqsr_bam_reader_open": (ctypes.c_int, [vp, vp, i64, i64, vp, pp]),
    "bqsr_bam_reader_destroy": (None, [vp]),
    "bqsr_bam_reader_members": (ctypes.c_int, [vp, vp, i64]),
    "bqsr_bam_reader_seek": (ctypes.c_int, [vp, i64, i64]),
    "bqsr_bam_reader_next": (ctypes.c_int, [vp, i64, vp, ctypes.POINTER(BamWindow)]),
    "bqsr_bam_index_add_window": (ctypes.c_int, [vp, vp, vp]),
    "bqsr_bam_reader_filter": (ctypes.c_int, [vp, i32, i64, i64, i64, vp, i64p, ctypes.POINTER(i32)]),
    "bqsr_bam_reader_parse": (ctypes.c_int, [vp, vp, pp]),
    "bqsr_bam_reader_get_stats": (ctypes.c_int, [vp, ctypes.POINTER(BamReaderStats)]),
}
SYMBOLS = tuple(_SIG)


def _lib():
    return _capi.bind(_capi.lib(), _SIG)


# ---- the region syntax ----

def parse_region(text: str, names: Sequence[str]) -> Tuple[int, int, int]:
    """(refID, beg, end), 0-based and half open, of ``NAME``, ``NAME:BEG`` or
    ``NAME:BEG-END`` (1-based, inclusive, digits only).  The whole string is
    tried as an @SQ name first, so a name may hold ':'; END is clamped to 2^29;
    BEG < 1, BEG > END and ``*`` are refused (ValueError), as is a name the
    header does not have."""
    if text == "*":
        raise ValueError("-region *: unplaced reads are not reachable through a region")
    index = {}
    for i, n in enumerate(names):
        index.setdefault(n, i)
    if text in index:
        return index[text], 0, MAX_END
    name, sep, span = text.rpartition(":")
    if not sep or name not in index:
        raise ValueError("-region %s: no such reference in the header" % text)
    first, dash, last = span.partition("-")
    digits = lambda s: s.isascii() and s.isdigit()  # noqa: E731
    if not digits(first) or (dash and not digits(last)):
        raise ValueError("-region %s: the coordinates are BEG or BEG-END, digits only" % text)
    beg = int(first)
    end = min(int(last), MAX_END) if dash else MAX_END
    if beg < 1 or beg > end:
        raise ValueError("-region %s: BEG must be at least 1 and at most END (END is clamped to 2^29)" % text)
    return index[name], beg - 1, end


# ---- the BAM header, on the host ----

def _members(data):
    """(file offset, size, isize, header size) of the BGZF members of `data`, from its start"""
    p, n = 0, len(data)
    while p < n:
        if n - p < 18 or bytes(data[p:p + 4]) != b"\x1f\x8b\x08\x04":
            raise ValueError("not a BGZF member at byte %d" % p)
        xlen, = struct.unpack_from("<H", data, p + 10)
        size, q = None, p + 12
        while q + 4 <= p + 12 + xlen:
            sl, = struct.unpack_from("<H", data, q + 2)
            if bytes(data[q:q + 2]) == b"BC" and sl == 2:
                size = struct.unpack_from("<H", data, q + 4)[0] + 1
            q += 4 + sl
        if size is None or p + size > n or size < 12 + xlen + 8:
            raise ValueError("BGZF member at byte %d: no BSIZE, or the file ends inside it" % p)
        yield p, size, struct.unpack_from("<I", data, p + size - 4)[0], 12 + xlen
        p += size


def bam_header(data) -> Tuple[bytes, List[str], List[int]]:
    """(SAM header text, reference names, reference lengths) of a BAM's bytes,
    inflating only the members the header spans (zlib on the host: what a
    refusal before any device work needs)."""
    raw = b""
    gen = _members(data)
    while True:
        if len(raw) >= 12:
            if raw[:4] != b"BAM\1":
                raise ValueError("no BAM magic")
            l_text, = struct.unpack_from("<i", raw, 4)
            p = 8 + l_text
            if l_text >= 0 and len(raw) >= p + 4:
                n_ref, = struct.unpack_from("<i", raw, p)
                p += 4
                names, lens = [], []
                while len(names) < n_ref and len(raw) >= p + 4:
                    l_name, = struct.unpack_from("<i", raw, p)
                    if l_name < 1:
                        raise ValueError("bad reference name in the BAM header")
                    if len(raw) < p + 4 + l_name + 4:
                        break
                    names.append(raw[p + 4:p + 4 + l_name - 1].decode("latin-1"))
                    lens.append(struct.unpack_from("<i", raw, p + 4 + l_name)[0])
                    p += 8 + l_name
                if len(names) == n_ref:
                    return raw[8:8 + l_text].rstrip(b"\0"), names, lens
            elif l_text < 0:
                raise ValueError("bad header length in the BAM header")
        try:
            off, size, _isize, hdr = next(gen)
        except StopIteration:
            raise ValueError("the BAM header is truncated") from None
        try:
            raw += zlib.decompress(bytes(data[off + hdr:off + size - 8]), -15)
        except zlib.error as e:
            raise ValueError("the BGZF member at byte %d, which holds the BAM header, does not inflate: %s"
                             % (off, e)) from None


# ---- the .bai reader ----

def reg2bins(beg: int, end: int) -> List[int]:
    """every bin that may hold a record overlapping [beg, end) (SAM spec §5.3)"""
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(first + (beg >> shift), first + (end >> shift) + 1)
    return out


class BaiIndex:
    """A .bai file's bins, chunks and linear index, read trusting only the
    spec: any chunking of a bin, records of small bins kept in a parent bin, a
    reference without a linear index (the lower bound is 0 then), pseudo-bin
    37450 (kept apart in ``.meta``, never queried), the optional n_no_coor.
    ValueError for bytes that do not parse."""

    def __init__(self, bai: bytes):
        def need(p, k):
            if p + k > len(bai):
                raise ValueError("the .bai index is truncated at byte %d" % len(bai))
        if bai[:4] != b"BAI\1":
            raise ValueError("not a .bai index (no BAI magic)")
        need(4, 4)
        n_ref, = struct.unpack_from("<i", bai, 4)
        if n_ref < 0:
            raise ValueError("the .bai index has a negative reference count")
        p = 8
        self.bins: List[Dict[int, List[Tuple[int, int]]]] = []
        self.linear: List[List[int]] = []
        self.meta: List[Optional[List[Tuple[int, int]]]] = []
        for _ in range(n_ref):
            need(p, 4)
            n_bin, = struct.unpack_from("<i", bai, p)
            p += 4
            bins: Dict[int, List[Tuple[int, int]]] = {}
            meta = None
            if n_bin < 0:
                raise ValueError("the .bai index has a negative bin count")
            for _ in range(n_bin):
                need(p, 8)
                b, n_chunk = struct.unpack_from("<Ii", bai, p)
                p += 8
                if n_chunk < 0:
                    raise ValueError("the .bai index has a negative chunk count")
                need(p, 16 * n_chunk)
                chunks = [struct.unpack_from("<QQ", bai, p + 16 * k) for k in range(n_chunk)]
                p += 16 * n_chunk
                if b == PSEUDO_BIN:
                    meta = chunks
                elif b > PSEUDO_BIN:
                    raise ValueError("the .bai index has bin %d, above the last one" % b)
                else:
                    bins.setdefault(b, []).extend(chunks)
            need(p, 4)
            n_intv, = struct.unpack_from("<i", bai, p)
            p += 4
            if n_intv < 0:
                raise ValueError("the .bai index has a negative window count")
            need(p, 8 * n_intv)
            self.linear.append(list(struct.unpack_from("<%dQ" % n_intv, bai, p)))
            p += 8 * n_intv
            self.bins.append(bins)
            self.meta.append(meta)
        self.n_no_coor = None
        if p + 8 == len(bai):
            self.n_no_coor, = struct.unpack_from("<Q", bai, p)
        elif p != len(bai):
            raise ValueError("the .bai index has %d bytes after its last reference" % (len(bai) - p))
        self.n_ref = n_ref

    @classmethod
    def read(cls, path: str) -> "BaiIndex":
        with open(path, "rb") as fh:
            return cls(fh.read())

    def validate(self, n_ref: int, file_size: int) -> None:
        """ValueError unless the index is of a BAM with n_ref references and file_size bytes"""
        if self.n_ref != n_ref:
            raise ValueError("the .bai index has %d references, the BAM header %d: not this file's index"
                             % (self.n_ref, n_ref))
        for bins in self.bins:
            for b, chunks in bins.items():
                for u, v in chunks:
                    if u > v or (v >> 16) > file_size or (u >> 16) >= file_size:
                        raise ValueError("the .bai index has a chunk of bin %d that points outside the file" % b)

    def chunks(self, rid: int, beg: int, end: int) -> List[Tuple[int, int]]:
        """The chunks to read for [beg, end) of reference rid: those of
        reg2bins' bins that end above the linear index's lower bound, sorted,
        and merged where they touch or overlap (so a record is read once)."""
        lin = self.linear[rid]
        w = beg >> 14
        low = 0 if not lin else lin[min(w, len(lin) - 1)]
        got = []
        bins = self.bins[rid]
        for b in reg2bins(beg, end):
            got += [c for c in bins.get(b, ()) if c[1] > low and c[1] > c[0]]
        got.sort()
        out: List[List[int]] = []
        for u, v in got:
            if out and u <= out[-1][1]:
                out[-1][1] = max(out[-1][1], v)
            else:
                out.append([u, v])
        return [(u, v) for u, v in out]


def find_index(path: str, bai: Optional[str] = None) -> str:
    """IN.bam.bai, else IN.bai, else the path given; ValueError when there is none"""
    if bai is not None:
        if not os.path.isfile(bai):
            raise ValueError("no index file %s (python -m adam_amd.bam_index IN.bam writes one)" % bai)
        return bai
    stem = path[:-4] if path.endswith(".bam") else path
    for cand in (path + ".bai", stem + ".bai"):
        if os.path.isfile(cand):
            return cand
    raise ValueError("-region needs an index: no %s.bai beside the input; `python -m adam_amd.bam_index %s` writes one"
                     % (path, path))


# ---- the windowed reader ----

class _Reader:
    """bqsr_bam_reader over a mapped file (kept alive here)"""

    def __init__(self, data, ctx, piece_bytes: int):
        self.L = _lib()
        self.view = np.frombuffer(data, np.uint8) if len(data) else np.zeros(0, np.uint8)
        self.h = ctypes.c_void_p()
        try:
            check(self.L.bqsr_bam_reader_open(ctx.handle, self.view.ctypes.data if self.view.size else None,
                                              self.view.size, int(piece_bytes), None, ctypes.byref(self.h)))
        except BaseException:
            self.view = None  # (the caller closes the map: no export of it may outlive this frame)
            raise

    def close(self):
        h, self.h = self.h, None
        if h:
            self.L.bqsr_bam_reader_destroy(h)
        self.view = None

    def stats(self) -> BamReaderStats:
        st = BamReaderStats()
        check(self.L.bqsr_bam_reader_get_stats(self.h, ctypes.byref(st)))
        return st

    def members(self) -> np.ndarray:
        """[n_members + 1, 2] (stream start, file offset), the terminal entry last"""
        n = self.stats().members_total
        t = np.zeros(2 * (n + 1), np.uint64)
        check(self.L.bqsr_bam_reader_members(self.h, t.ctypes.data, t.size))
        return t.reshape(-1, 2)

    def next(self, end_member: int) -> BamWindow:
        w = BamWindow()
        check(self.L.bqsr_bam_reader_next(self.h, int(end_member), None, ctypes.byref(w)))
        return w


def _piece(piece_bytes) -> int:
    piece = DEFAULT_PIECE_BYTES if piece_bytes is None else int(piece_bytes)
    if not 1 <= piece <= 1 << 31:
        raise ValueError("-piece_bytes must be 1 .. 2^31")
    return piece


def index_bytes(data, ctx, piece_bytes: Optional[int] = None) -> Tuple[bytes, dict]:
    """(the .bai file's bytes, stats) of a BAM's bytes; BQSRError for a file
    that is refused (``.read``: the record's ordinal in the file)"""
    from .transform import BAM_INDEX_KERNELS, BamIndexSizes, _index_lib
    L, X = _lib(), _index_lib()
    rd = _Reader(data, ctx, _piece(piece_bytes))
    idx = ctypes.c_void_p()
    try:
        st = rd.stats()
        table = rd.members()
        if len(table) > 1 and int(table[-1, 0]) - int(table[-2, 0]) == 65536:
            raise _capi.BQSRError(_capi.UNSUPPORTED, "BAM index: the file has no EOF marker and its last member inflates "
                                  "to 65536 bytes: the stream's end has no virtual offset")
        check(X.bqsr_bam_index_create(ctx.handle, st.n_ref, ctypes.byref(idx)))
        while True:
            w = rd.next(st.members_total)
            if w.n_records:
                check(L.bqsr_bam_index_add_window(idx, rd.h, None))
            if w.done:
                break
        check(X.bqsr_bam_index_set_members(idx, table.ctypes.data, len(table) - 1, None))
        check(X.bqsr_bam_index_finish(idx, None))
        sz = BamIndexSizes()
        check(X.bqsr_bam_index_size(idx, ctypes.byref(sz)))
        buf = np.empty(max(1, sz.bytes), np.uint8)
        check(X.bqsr_bam_index_bytes(idx, buf.ctypes.data, sz.bytes))
        st = rd.stats()
        stats = {"reads": int(st.records_seen), "members_total": int(st.members_total),
                 "members_read": int(st.members_read), "stream_bytes": int(st.stream_bytes),
                 "windows_device": int(st.windows_device), "windows_host": int(st.windows_host),
                 "members_host": int(st.members_host), "index_bytes": int(sz.bytes), "index_chunks": int(sz.n_chunks), "index_bins": int(sz.n_bins),
                 "index_device_bytes": int(sz.device_bytes),
                 "index_ms": _capi.stage_times(X.bqsr_bam_index_kernel_times, BAM_INDEX_KERNELS, idx, array=True)}
        return buf[:sz.bytes].tobytes(), stats
    finally:
        if idx:
            X.bqsr_bam_index_destroy(idx)
        rd.close()


def bam_index(path: str, out: Optional[str] = None, overwrite: bool = False, piece_bytes: Optional[int] = None,
              device: int = 0) -> dict:
    """Write the .bai index of the BAM at `path` to `out` (default: path +
    ".bai"), through ``out.partial`` and a rename.  An existing output needs
    overwrite.  A refused file (not in coordinate order, an end above 2^29, a
    damaged member, a truncated record, not a BAM) raises BQSRError naming the
    record and leaves no file; what was at `out` stays."""
    from . import bqsr
    from .adam_save import check_out
    from .inputs import is_bam
    out = path + ".bai" if out is None else out
    piece = _piece(piece_bytes)
    check_out(out, overwrite, False)
    t0 = time.perf_counter()
    with open(path, "rb") as fh:
        data = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ) if os.path.getsize(path) else b""
    try:
        if not is_bam(data):
            raise _capi.BQSRError(_capi.SAM_PARSE, "%s is not a BAM file (no BGZF magic)" % path)
        bai, stats = index_bytes(data, bqsr.Context.get(device), piece)
    finally:
        if isinstance(data, mmap.mmap):
            data.close()
    tmp = out + ".partial"
    try:
        with open(tmp, "wb") as fh:
            fh.write(bai)
        os.replace(tmp, out)
    except BaseException:
        if os.path.lexists(tmp):
            os.unlink(tmp)
        raise
    stats["output"] = out
    stats["seconds_index"] = time.perf_counter() - t0
    return stats


# ---- a region through the index ----

def region_text(data, ctx, index: BaiIndex, rid: int, beg: int, end: int, piece_bytes: Optional[int] = None):
    """(SamText, stats) of the records of reference rid that overlap [beg,
    end): per merged chunk of the index, windows from the member of its u
    (first record at u's offset in it) to the member of its v; the device
    filter keeps the overlapping records before v; the kept records of all
    windows, in file order, are parsed as bqsr_bam_parse parses a file."""
    from .sam import SamText
    L = _lib()
    rd = _Reader(data, ctx, _piece(piece_bytes))
    try:
        table = rd.members()
        starts, offs = table[:-1, 0], table[:-1, 1]
        size = int(table[-1, 1])

        def member(coffset: int) -> int:
            m = int(np.searchsorted(offs, coffset))
            if m >= len(offs) or int(offs[m]) != coffset:
                if coffset == size:  # (an end expressed past the last member)
                    return len(offs)
                raise ValueError("the .bai index has a chunk at file offset %d, where no BGZF member starts: not this "
                                 "file's index" % coffset)
            return m

        kept, done = ctypes.c_int64(), ctypes.c_int32()
        over = False
        for u, v in index.chunks(rid, beg, end):
            if over:
                break
            mu, mv = member(u >> 16), member(v >> 16)
            if mu >= len(offs):
                continue
            limit = (int(starts[mv]) if mv < len(offs) else int(table[-1, 0])) + (v & 0xFFFF)
            check(L.bqsr_bam_reader_seek(rd.h, mu, u & 0xFFFF))
            while True:
                w = rd.next(mv + 1)
                if w.n_records:
                    check(L.bqsr_bam_reader_filter(rd.h, rid, beg, end, limit, None, ctypes.byref(kept),
                                                   ctypes.byref(done)))
                    if done.value:
                        over = done.value == 2
                        break
                if w.done or w.next_pos >= limit:
                    break
        h = ctypes.c_void_p()
        check(L.bqsr_bam_reader_parse(rd.h, None, ctypes.byref(h)))
        sam = SamText.adopt(h, ctx)
        sam.bam = True
        st = rd.stats()
        return sam, {"members_read": int(st.members_read), "members_total": int(st.members_total),
                     "records_seen": int(st.records_seen), "records_kept": int(st.records_kept),
                     "windows_device": int(st.windows_device), "windows_host": int(st.windows_host),
                     "members_host": int(st.members_host), "filter_ms": float(st.filter_ms)}
    finally:
        rd.close()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="adam_amd.bam_index", description=__doc__.split("\n\n")[0])
    ap.add_argument("input", help="a BAM file in coordinate order")
    ap.add_argument("-output", default=None, help="the index file (default: INPUT.bai)")
    ap.add_argument("-overwrite", action="store_true", help="replace an existing index file")
    ap.add_argument("-piece_bytes", type=int, default=DEFAULT_PIECE_BYTES,
                    help="inflated bytes per window on the device (default 1 GiB)")
    a = ap.parse_args(argv)
    from .inputs import report
    t0 = time.perf_counter()
    try:
        st = bam_index(a.input, a.output, a.overwrite, a.piece_bytes)
    except (ValueError, FileExistsError, FileNotFoundError) as e:
        print("adam_amd.bam_index: %s" % e, file=sys.stderr)
        return 2
    st.pop("seconds_index", None)
    report(st, t0)
    return 0


if __name__ == "__main__":
    sys.exit(main())
