"""BAM files with chosen BGZF member cuts, for the tests of
adam_amd.bam_index and ``SamInput(region=...)``: a SAM text's BAM stream
(tests/_bam_ref.stream) packed into members at the cuts a test names, and
.bai indexes altered in ways the spec allows.

``CUTS`` maps a name to ``cut(stream, record_ends) -> [member payloads]``;
``bam_file(text, cut)`` is the file; ``coarse`` / ``no_linear`` / ``folded``
rewrite a parsed index.
"""
from __future__ import annotations

import struct
import zlib
from typing import Callable, Dict, List

import _bai_gen as G
import _bai_ref as R
import _bam_ref as B

EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def member(raw: bytes, stored: bool = False) -> bytes:
    """one BGZF member of `raw` (at most 65536 bytes, and a member of at most 65536)"""
    assert len(raw) <= 65536
    if stored:
        body = b"\x01" + struct.pack("<HH", len(raw), len(raw) ^ 0xFFFF) + raw if len(raw) < 65536 else None
        if body is None:  # (two stored blocks)
            body = (b"\x00" + struct.pack("<HH", 65535, 0) + raw[:65535] + b"\x01" + struct.pack("<HH", 1, 0xFFFE)
                    + raw[65535:])
    else:
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = c.compress(raw) + c.flush()
    size = 18 + len(body) + 8
    assert size <= 65536
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", size - 1) + body
            + struct.pack("<II", zlib.crc32(raw), len(raw)))


def by_size(n: int):
    def cut(stream: bytes, ends: List[int]) -> List[bytes]:
        return [stream[a:a + n] for a in range(0, len(stream), n)]
    return cut


def at_records(stream: bytes, ends: List[int]) -> List[bytes]:
    """members end on record boundaries (the header is a member of its own), a
    member taking records while it stays within 60000 bytes; a longer record is
    cut by size"""
    out, a, last = [], 0, 0
    for e in ends:
        if e - a > 60000 and last > a:
            out.append(stream[a:last])
            a = last
        while e - a > 60000:
            out.append(stream[a:a + 60000])
            a += 60000
        last = e
    out.append(stream[a:])
    return [m for m in out if m]


def empty_in_the_middle(stream: bytes, ends: List[int]) -> List[bytes]:
    parts = by_size(20000)(stream, ends)
    k = len(parts) // 2
    return parts[:k] + [b""] + parts[k:]


CUTS: Dict[str, Callable] = {
    "project": by_size(65280),
    "records": at_records,
    "small": by_size(1000),
    "empty_member": empty_in_the_middle,
    "stored": by_size(30000),
    "no_eof": by_size(50000),
}

LONG_HEADER = G.HEAD + b"".join(b"@CO\tcomment line %04d %s\n" % (i, b"x" * 60) for i in range(60))


def long_header() -> bytes:
    """a header of several kB of @CO lines: it spans members under the 1000-byte cut"""
    return LONG_HEADER + b"".join(G.lines(G.bins_and_windows()))


SHAPES = dict(G.SHAPES, long_header=long_header)
PIECES = (None, 3000, 70000)  # the whole file as one window; windows that end inside records and the header

_files: Dict[tuple, bytes] = {}
_texts: Dict[str, bytes] = {}


def text_of(shape: str) -> bytes:
    if shape not in _texts:
        _texts[shape] = SHAPES[shape]()
    return _texts[shape]


def pack(stream: bytes, ends: List[int], cut: str) -> bytes:
    parts = CUTS[cut](stream, ends)
    assert b"".join(parts) == stream
    data = b"".join(member(p, stored=cut == "stored") for p in parts)
    return data if cut == "no_eof" else data + EOF


def bam_file(shape: str, cut: str) -> bytes:
    """the BAM of SHAPES[shape] under CUTS[cut] (made once)"""
    key = (shape, cut)
    if key not in _files:
        text = text_of(shape)
        head = B.header(text)[0]
        ends, p = [len(head)], len(head)
        for r in B.records(text):
            p += len(r)
            ends.append(p)
        _files[key] = pack(head + b"".join(B.records(text)), ends, cut)
    return _files[key]


# ---- altered indexes ----

def serialize(P: dict) -> bytes:
    out = [b"BAI\1", struct.pack("<i", len(P["refs"]))]
    for ref in P["refs"]:
        out.append(struct.pack("<i", len(ref["order"])))
        for b in ref["order"]:
            out.append(struct.pack("<Ii", b, len(ref["bins"][b])))
            out += [struct.pack("<QQ", *c) for c in ref["bins"][b]]
        out.append(struct.pack("<i", len(ref["linear"])))
        out += [struct.pack("<Q", w) for w in ref["linear"]]
    out.append(struct.pack("<Q", P["n_no_coor"]))
    return b"".join(out)


def coarse(bai: bytes) -> bytes:
    """every bin's chunks merged into one"""
    P = R.parse_bai(bai)
    for ref in P["refs"]:
        for b, c in ref["bins"].items():
            if b != R.PSEUDO_BIN and c:
                ref["bins"][b] = [(min(x[0] for x in c), max(x[1] for x in c))]
    return serialize(P)


def no_linear(bai: bytes) -> bytes:
    P = R.parse_bai(bai)
    for ref in P["refs"]:
        ref["linear"] = []
    return serialize(P)


def folded(bai: bytes) -> bytes:
    """leaf bins folded into their parents: a leaf's chunks join its parent's, sorted"""
    P = R.parse_bai(bai)
    for ref in P["refs"]:
        for b in [b for b in ref["order"] if 4681 <= b < R.PSEUDO_BIN]:
            parent = 585 + ((b - 4681) >> 3)
            if parent not in ref["bins"]:
                ref["bins"][parent] = []
                ref["order"].append(parent)
            ref["bins"][parent] = sorted(ref["bins"][parent] + ref["bins"].pop(b))
            ref["order"].remove(b)
        meta = [b for b in ref["order"] if b == R.PSEUDO_BIN]
        ref["order"] = sorted(b for b in ref["order"] if b != R.PSEUDO_BIN) + meta
    return serialize(P)


ALTERED = {"coarse": coarse, "no_linear": no_linear, "folded": folded}
