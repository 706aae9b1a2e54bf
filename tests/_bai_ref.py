"""The .bai index restated from the SAM spec (§5.2, §5.3) and the rules
include/adam_sam.h states at bqsr_bam_index_create, working from a finished
BAM file alone: the yardstick of the device index's tests
(tests/test_bai_ref.py pins it).

``bai_of_bam(bam)`` walks the BGZF members by BSIZE, inflates them with zlib,
walks the records with their virtual offsets and builds the index serially;
``BaiRefusal`` (``.status``, ``.read``) for an output that is not in coordinate
order or a record that ends above 2^29.  ``parse_bai`` and ``query`` are a
reader that decides what to read from the index alone: the spec's reg2bins,
the linear index as the lower bound, the chunks.
"""
from __future__ import annotations

import bisect
import struct
import zlib
from typing import Dict, List, Tuple

UNSORTED, UNSUPPORTED = "UNSORTED", "UNSUPPORTED"
PSEUDO_BIN = 37450
MAX_END = 1 << 29


class BaiRefusal(Exception):
    def __init__(self, status: str, read: int):
        super().__init__("%s: read %d" % (status, read))
        self.status = status
        self.read = read


def reg2bin(beg: int, end: int) -> int:
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def reg2bins(beg: int, end: int) -> List[int]:
    """every bin that may hold a record overlapping [beg, end) (§5.3)"""
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(first + (beg >> shift), first + (end >> shift) + 1)
    return out


class Stream:
    """the members of a BAM file: file offsets, inflated bytes, stream starts"""

    def __init__(self, bam: bytes):
        self.file_off: List[int] = []
        self.raw: List[bytes] = []
        p = 0
        while p < len(bam):
            assert bam[p:p + 4] == b"\x1f\x8b\x08\x04" and bam[p + 12:p + 16] == b"BC\x02\x00", p
            size = struct.unpack_from("<H", bam, p + 16)[0] + 1
            raw = zlib.decompress(bam[p + 18:p + size - 8], -15)
            assert len(raw) == struct.unpack_from("<I", bam, p + size - 4)[0]
            self.file_off.append(p)
            self.raw.append(raw)
            p += size
        assert p == len(bam)
        self.start = [0]
        for r in self.raw:
            self.start.append(self.start[-1] + len(r))
        self.data = b"".join(self.raw)
        self.member_of = {o: m for m, o in enumerate(self.file_off)}

    def voff(self, p: int) -> int:
        """p lies in the member with start[m] <= p < start[m + 1]; the end of
        the stream lies in the last member, the EOF marker"""
        m = min(bisect.bisect_right(self.start, p) - 1, len(self.raw) - 1)
        return self.file_off[m] << 16 | (p - self.start[m])

    def pos(self, v: int) -> int:
        return self.start[self.member_of[v >> 16]] + (v & 0xFFFF)


def header_end(data: bytes) -> Tuple[int, int]:
    """(where the records start, n_ref) of an inflated BAM stream"""
    assert data[:4] == b"BAM\1"
    p = 8 + struct.unpack_from("<i", data, 4)[0]
    n_ref = struct.unpack_from("<i", data, p)[0]
    p += 4
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<i", data, p)[0]
    return p, n_ref


def record_at(data: bytes, p: int):
    """(refID, beg, end, flag, next position) of the record at p, with the
    index's interval: beg clamped to 0, end at least beg + 1"""
    bs, rid, pos, _l, _q, _b, n_cig, flag = struct.unpack_from("<iiiBBHHH", data, p)
    l_name = data[p + 12]
    ref_len = 0
    for w in struct.unpack_from("<%dI" % n_cig, data, p + 36 + l_name):
        if w & 15 in (0, 2, 3, 7, 8):  # M D N = X
            ref_len += w >> 4
    end = pos + (ref_len if ref_len > 0 else 1)
    beg = max(pos, 0)
    return rid, beg, max(end, beg + 1), flag, p + 4 + bs


def walk(bam: bytes):
    """(Stream, n_ref, [(refID, beg, end, flag, u, v)]) of a BAM file"""
    S = Stream(bam)
    p, n_ref = header_end(S.data)
    recs = []
    while p < len(S.data):
        rid, beg, end, flag, q = record_at(S.data, p)
        recs.append((rid, beg, end, flag, S.voff(p), S.voff(q)))
        p = q
    assert p == len(S.data)
    return S, n_ref, recs


def bai_of_bam(bam: bytes) -> bytes:
    _, n_ref, recs = walk(bam)
    refs: List[dict] = [dict(bins={}, lin={}, n=0, mapped=0, unmapped=0, first=0, last=0, max_end=0)
                        for _ in range(n_ref)]
    n_no_coor = 0
    prev = None
    for i, (rid, beg, end, flag, u, v) in enumerate(recs):
        if rid >= 0:
            if prev is not None and (prev[0] < 0 or rid < prev[0] or (rid == prev[0] and beg < prev[1])):
                raise BaiRefusal(UNSORTED, i)
            if end > MAX_END:
                raise BaiRefusal(UNSUPPORTED, i)
        prev = (rid, beg)
        if rid < 0:
            n_no_coor += 1
            continue
        R = refs[rid]
        chunks = R["bins"].setdefault(reg2bin(beg, end), [])
        if chunks and chunks[-1][1] >> 16 >= u >> 16:
            chunks[-1][1] = v
        else:
            chunks.append([u, v])
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            R["lin"][w] = min(R["lin"].get(w, u), u)
        if R["n"] == 0:
            R["first"] = u
        R["n"] += 1
        R["last"] = v
        R["unmapped" if flag & 4 else "mapped"] += 1
        R["max_end"] = max(R["max_end"], end)
    out = [b"BAI\1", struct.pack("<i", n_ref)]
    for R in refs:
        if R["n"] == 0:
            out.append(struct.pack("<ii", 0, 0))
            continue
        out.append(struct.pack("<i", len(R["bins"]) + 1))
        for b in sorted(R["bins"]):
            out.append(struct.pack("<Ii", b, len(R["bins"][b])))
            out += [struct.pack("<QQ", c[0], c[1]) for c in R["bins"][b]]
        out.append(struct.pack("<IiQQQQ", PSEUDO_BIN, 2, R["first"], R["last"], R["mapped"], R["unmapped"]))
        n_intv = 1 + ((R["max_end"] - 1) >> 14)
        out.append(struct.pack("<i", n_intv))
        last = 0
        for w in range(n_intv):
            last = R["lin"].get(w, last)
            out.append(struct.pack("<Q", last))
    out.append(struct.pack("<Q", n_no_coor))
    return b"".join(out)


def parse_bai(bai: bytes) -> dict:
    assert bai[:4] == b"BAI\1"
    n_ref, = struct.unpack_from("<i", bai, 4)
    p = 8
    refs = []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", bai, p)
        p += 4
        bins: Dict[int, List[Tuple[int, int]]] = {}
        order = []
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", bai, p)
            p += 8
            assert b not in bins
            bins[b] = [struct.unpack_from("<QQ", bai, p + 16 * k) for k in range(n_chunk)]
            order.append(b)
            p += 16 * n_chunk
        n_intv, = struct.unpack_from("<i", bai, p)
        p += 4
        lin = list(struct.unpack_from("<%dQ" % n_intv, bai, p))
        p += 8 * n_intv
        refs.append(dict(bins=bins, order=order, linear=lin))
    n_no_coor, = struct.unpack_from("<Q", bai, p)
    assert p + 8 == len(bai)
    return dict(refs=refs, n_no_coor=n_no_coor)


def query(bam: bytes, bai: bytes, rid: int, beg: int, end: int) -> List[int]:
    """the ordinals of the records of reference `rid` that overlap [beg, end),
    reading only the chunks the index names (a record's ordinal by its u)"""
    S, _, recs = walk(bam)
    ordinal = {r[4]: i for i, r in enumerate(recs)}
    R = parse_bai(bai)["refs"][rid]
    lin = R["linear"]
    if beg >> 14 >= len(lin):  # past every record's end
        return []
    min_off = lin[beg >> 14]
    hits = set()
    for b in reg2bins(beg, end):
        for cb, ce in R["bins"].get(b, ()):
            if ce <= min_off:
                continue
            p = S.pos(cb)
            while S.voff(p) < ce:
                r_id, r_beg, r_end, _f, q = record_at(S.data, p)
                u = S.voff(p)
                if u >= min_off and r_id == rid and r_beg < end and r_end > beg:
                    hits.add(ordinal[u])
                p = q
    return sorted(hits)


def scan(bam: bytes, rid: int, beg: int, end: int) -> List[int]:
    """the same by looking at every record"""
    return [i for i, r in enumerate(walk(bam)[2]) if r[0] == rid and r[1] < end and r[2] > beg]
