"""An independent BAM encoder written from the SAM spec (§4.2, §5.3), the
yardstick of the device encoder's tests (tests/test_bam_ref.py pins it).

``records(text)`` gives the BAM records of a SAM text, ``header(text)`` the
BAM header, ``stream(text)`` both.  Field rules:

  refID the @SQ index of RNAME ("*": -1); pos POS - 1; l_read_name QNAME + 1;
  bin reg2bin(pos, end) with arithmetic shifts, end = pos + the CIGAR's
  reference length (M D N = X), pos + 1 when that is 0 or CIGAR is "*";
  next_refID "=": refID, "*": -1; SEQ as 4-bit codes of "=ACMGRSVTWYHKDBN"
  (upper-cased, anything else 15, high nibble first); QUAL - 33 or l_seq
  bytes of 0xFF for "*"; tags in input order: A, i as the smallest of
  c C s S i I (signed first), f as binary32 correctly rounded from the
  decimal text, Z / H with a NUL, B arrays as type, int32 count, values.

What BAM cannot hold raises ``BamRefusal`` with ``.read`` the record's index.
"""
from __future__ import annotations

import re
import struct
from fractions import Fraction
from typing import Dict, List, Tuple

SEQ_CODES = "=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"
INT_TYPES = (("c", "<b", -128, 127), ("C", "<B", 0, 255), ("s", "<h", -32768, 32767), ("S", "<H", 0, 65535),
             ("i", "<i", -2 ** 31, 2 ** 31 - 1), ("I", "<I", 0, 2 ** 32 - 1))
_INT = re.compile(rb"[-+]?[0-9]+\Z")
_FLOAT = re.compile(rb"[-+]?([0-9]+\.?[0-9]*|\.[0-9]+)([eE][-+]?[0-9]+)?\Z")
_HEX = re.compile(rb"([0-9A-Fa-f]{2})*\Z")


class BamRefusal(Exception):
    def __init__(self, msg: str, read: int = -1):
        super().__init__(msg)
        self.read = read


def reg2bin(beg: int, end: int) -> int:
    """SAM spec §5.3 (Python's >> is arithmetic)"""
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


def int_tag(v: int) -> bytes:
    """type letter + value of an 'i' tag: the smallest type, signed first"""
    for t, fmt, lo, hi in INT_TYPES:
        if lo <= v <= hi:
            return t.encode() + struct.pack(fmt, v)
    raise BamRefusal("an 'i' value outside [-2^31, 2^32 - 1]")


def float32_bits(text: bytes) -> bytes:
    """binary32 of a decimal text, correctly rounded (round half to even) by
    exact rational arithmetic -- what C strtof gives"""
    s = text.decode("ascii")
    low = s.lstrip("+-").lower()
    neg = s.startswith("-")
    if low in ("inf", "infinity"):
        return struct.pack("<I", 0xFF800000 if neg else 0x7F800000)
    if low == "nan":
        return struct.pack("<f", float("nan"))
    if not _FLOAT.match(text):
        raise BamRefusal("an 'f' value that is not a number")
    x = abs(Fraction(s))
    sign = 0x80000000 if neg else 0
    if x == 0:
        return struct.pack("<I", sign)
    # x = m * 2^e with 2^23 <= m < 2^24 (normal) or e = -149 (subnormal)
    e = x.numerator.bit_length() - x.denominator.bit_length() - 24
    while x / Fraction(2) ** e >= 1 << 24:
        e += 1
    while x / Fraction(2) ** e < 1 << 23:
        e -= 1
    e = max(e, -149)
    q = x / Fraction(2) ** e
    m = q.numerator // q.denominator
    rem = q - m
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and m & 1):
        m += 1
    if m == 1 << 24:
        m >>= 1
        e += 1
    if e > 104:  # above the largest finite binary32
        return struct.pack("<I", sign | 0x7F800000)
    if m < 1 << 23:  # subnormal (e == -149)
        return struct.pack("<I", sign | m)
    return struct.pack("<I", sign | ((e + 150) << 23) | (m - (1 << 23)))


def _tag(t: bytes) -> bytes:
    if len(t) < 5 or t[2:3] != b":" or t[4:5] != b":":
        raise BamRefusal("an optional field that is not TG:T:value")
    tag, typ, val = t[:2], t[3:4], t[5:]
    if typ == b"A":
        if len(val) != 1:
            raise BamRefusal("an A value that is not one byte")
        return tag + b"A" + val
    if typ == b"i":
        if not _INT.match(val):
            raise BamRefusal("an 'i' value that is not a number")
        return tag + int_tag(int(val))
    if typ == b"f":
        return tag + b"f" + float32_bits(val)
    if typ == b"Z":
        return tag + b"Z" + val + b"\0"
    if typ == b"H":
        if not _HEX.match(val):
            raise BamRefusal("an odd-length or non-hex H")
        return tag + b"H" + val + b"\0"
    if typ == b"B":
        parts = val.split(b",")
        et, vals = parts[0], parts[1:]
        if et == b"f":
            body = b"".join(float32_bits(v) for v in vals)
        else:
            spec = {t: (fmt, lo, hi) for t, fmt, lo, hi in INT_TYPES}.get(et.decode("latin-1"))
            if spec is None:
                raise BamRefusal("a B array of an unknown element type")
            body = b""
            for v in vals:
                if not _INT.match(v):
                    raise BamRefusal("a B value that is not a number")
                if not spec[1] <= int(v) <= spec[2]:
                    raise BamRefusal("a B value outside its element type")
                body += struct.pack(spec[0], int(v))
        return tag + b"B" + et + struct.pack("<i", len(vals)) + body
    raise BamRefusal("an unknown tag type letter")


def _i32(v: int, what: str) -> int:
    if not -2 ** 31 <= v <= 2 ** 31 - 1:
        raise BamRefusal(what + " outside int32")
    return v


def record(line: bytes, ref_id: Dict[bytes, int]) -> bytes:
    f = line.split(b"\t")
    qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = f[:11]
    if len(qname) > 254:
        raise BamRefusal("QNAME longer than 254 bytes")
    flag, mapq = int(flag), int(mapq)
    if not 0 <= flag <= 65535 or not 0 <= mapq <= 255:
        raise BamRefusal("FLAG or MAPQ outside its field")
    if rname == b"*":
        rid = -1
    elif rname in ref_id:
        rid = ref_id[rname]
    else:
        raise BamRefusal("RNAME is no @SQ name")
    pos = _i32(int(pos) - 1, "POS")
    ops: List[int] = []
    if cigar != b"*":
        for n, op in re.findall(rb"([0-9]+)([MIDNSHP=X])", cigar):
            ops.append(int(n) << 4 | CIGAR_OPS.index(op.decode()))
    if len(ops) > 65535:
        raise BamRefusal("more than 65535 CIGAR elements")
    if rnext == b"=":
        nid = rid
    elif rnext == b"*":
        nid = -1
    elif rnext in ref_id:
        nid = ref_id[rnext]
    else:
        raise BamRefusal("RNEXT is no @SQ name")
    pnext = _i32(int(pnext) - 1, "PNEXT")
    tlen = _i32(int(tlen), "TLEN")
    l_seq = 0 if seq == b"*" else len(seq)
    packed = bytearray((l_seq + 1) // 2)
    for i in range(l_seq):
        c = chr(seq[i]).upper()
        code = SEQ_CODES.index(c) if c in SEQ_CODES else 15
        packed[i // 2] |= code << (0 if i % 2 else 4)
    if qual == b"*":
        q = b"\xff" * l_seq
    else:
        if len(qual) != l_seq or any(not 33 <= b <= 126 for b in qual):
            raise BamRefusal("QUAL differs from SEQ in length or has a byte outside '!'..'~'")
        q = bytes(b - 33 for b in qual)
    tags = b"".join(_tag(t) for t in f[11:])
    ref_len = sum(o >> 4 for o in ops if CIGAR_OPS[o & 15] in "MDN=X")
    end = pos + (ref_len if ref_len > 0 else 1)
    name = qname + b"\0"
    body = struct.pack("<iiBBHHHiiii", rid, pos, len(name), mapq, reg2bin(pos, end) & 0xFFFF, len(ops), flag, l_seq, nid,
                       pnext, tlen)
    body += name + b"".join(struct.pack("<I", o) for o in ops) + bytes(packed) + q + tags
    return struct.pack("<i", len(body)) + body


def _split(text: bytes) -> Tuple[List[bytes], List[bytes]]:
    lines = [l[:-1] if l.endswith(b"\r") else l for l in text.split(b"\n")]
    return [l for l in lines if l.startswith(b"@")], [l for l in lines if l and not l.startswith(b"@")]


def header(text: bytes) -> Tuple[bytes, Dict[bytes, int]]:
    """(BAM header, @SQ name -> index): magic, l_text, the header lines
    unchanged, n_ref, every @SQ as l_name, name, NUL, LN (0 when absent)"""
    head, _ = _split(text)
    refs = []
    for l in head:
        if l.split(b"\t")[0] == b"@SQ":
            kv = dict(x.split(b":", 1) for x in l.split(b"\t")[1:] if b":" in x)
            refs.append((kv[b"SN"], int(kv.get(b"LN", b"0"))))
    ref_id: Dict[bytes, int] = {}
    for i, (n, _) in enumerate(refs):
        ref_id.setdefault(n, i)
    htext = b"".join(l + b"\n" for l in head)
    raw = b"BAM\1" + struct.pack("<i", len(htext)) + htext + struct.pack("<i", len(refs))
    for n, ln in refs:
        raw += struct.pack("<i", len(n) + 1) + n + b"\0" + struct.pack("<i", ln)
    return raw, ref_id


def records(text: bytes) -> List[bytes]:
    _, ref_id = header(text)
    out = []
    for i, l in enumerate(_split(text)[1]):
        try:
            out.append(record(l, ref_id))
        except BamRefusal as e:
            raise BamRefusal("read %d: %s" % (i, e), i) from None
    return out


def stream(text: bytes) -> bytes:
    return header(text)[0] + b"".join(records(text))


# ---- walking a BAM stream back into fields (for field-by-field comparisons) ----

def parse_stream(raw: bytes):
    """(header text, [(name, LN)], [record dict]) of an inflated BAM stream"""
    assert raw[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", raw, 4)
    p = 8 + l_text
    text = raw[8:p]
    n_ref, = struct.unpack_from("<i", raw, p)
    p += 4
    refs = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", raw, p)
        name = raw[p + 4:p + 4 + l_name - 1]
        ln, = struct.unpack_from("<i", raw, p + 4 + l_name)
        refs.append((name, ln))
        p += 8 + l_name
    recs = []
    while p < len(raw):
        bs, = struct.unpack_from("<i", raw, p)
        recs.append(parse_record(raw[p + 4:p + 4 + bs]))
        p += 4 + bs
    assert p == len(raw)
    return text, refs, recs


def parse_record(b: bytes) -> dict:
    rid, pos, l_name, mapq, bin_, n_cig, flag, l_seq, nid, npos, tlen = struct.unpack_from("<iiBBHHHiiii", b, 0)
    p = 32
    name = b[p:p + l_name]
    p += l_name
    cigar = struct.unpack_from("<%dI" % n_cig, b, p)
    p += 4 * n_cig
    seq = b[p:p + (l_seq + 1) // 2]
    p += (l_seq + 1) // 2
    qual = b[p:p + l_seq]
    p += l_seq
    return dict(refID=rid, pos=pos, name=name, mapq=mapq, bin=bin_, cigar=cigar, flag=flag, l_seq=l_seq, seq=seq,
                qual=qual, next_refID=nid, next_pos=npos, tlen=tlen, tags=b[p:])


def bgzf_members(data: bytes):
    """every BGZF member of a file, checked (BC field and BSIZE, CRC32, ISIZE)
    and inflated: [(inflated bytes, member size)]"""
    import zlib
    out = []
    p = 0
    while p < len(data):
        assert data[p:p + 4] == b"\x1f\x8b\x08\x04", p
        xlen, = struct.unpack_from("<H", data, p + 10)
        assert xlen == 6 and data[p + 12:p + 16] == b"BC\x02\x00", "the BC extra field"
        bsize, = struct.unpack_from("<H", data, p + 16)
        size = bsize + 1
        assert p + size <= len(data)
        d = zlib.decompressobj(-15)
        raw = d.decompress(data[p + 18:p + size - 8])
        assert d.eof and not d.unused_data
        crc, isize = struct.unpack_from("<II", data, p + size - 8)
        assert isize == len(raw) and crc == zlib.crc32(raw) & 0xFFFFFFFF
        out.append((raw, size))
        p += size
    return out
