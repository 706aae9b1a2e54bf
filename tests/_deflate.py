"""A bit-level DEFLATE (RFC 1951) and BGZF writer for the tests: streams are
written from explicit token lists and explicit code lengths, so a test can
emit forms a compressor never chooses -- and malformed ones.  zlib is the
judge of every stream written here (test_deflate_writer.py).

Tokens: an int is a literal byte; ``(length, distance)`` is a match written
with the usual symbols; ``("sym", lsym, lextra, dsym, dextra)`` writes the
length symbol ``lsym`` (257..287) and distance symbol ``dsym`` (0..31) with the
given extra-bit values as they are (``dsym`` None: no distance follows).
"""
import struct
import zlib

CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class BitWriter:
    """Bits LSB first into bytes (RFC 1951 §3.1.1)."""

    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):
        """A Huffman code of n bits, its most significant bit first."""
        for i in range(n - 1, -1, -1):
            self.bits((c >> i) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    @property
    def bitpos(self):
        return 8 * len(self.buf) + self.n

    def bytes(self):
        return bytes(self.buf) + (bytes([self.acc]) if self.n else b"")


def canonical(lengths):
    """The canonical codes (RFC 1951 §3.2.2) of a list of code lengths:
    [(code, length)] by symbol, (0, 0) for an unused one.  An over-subscribed
    list gets codes cut to their length (a stream of them is malformed)."""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        if l == 0:
            out.append((0, 0))
        else:
            out.append((nxt[l] & ((1 << l) - 1), l))
            nxt[l] += 1
    return out


def kraft(lengths):
    """Sum of 2^-l over the used lengths, in units of 2^-15 (32768: complete)."""
    return sum(1 << (15 - l) for l in lengths if l)


def length_symbol(length):
    """(symbol, extra bits, extra value) of a match length, 258 by symbol 285."""
    if length == 258:
        return 285, 0, 0
    s = max(i for i in range(28) if LEN_BASE[i] <= length)
    return 257 + s, LEN_EXTRA[s], length - LEN_BASE[s]


def dist_symbol(dist):
    s = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return s, DIST_EXTRA[s], dist - DIST_BASE[s]


def expand(tokens, prefix=b""):
    """The bytes a token list stands for (after `prefix`, which matches may reach into)."""
    out = bytearray(prefix)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
            continue
        if t[0] == "sym":
            _, ls, le, ds, de = t
            length, dist = LEN_BASE[ls - 257] + le, DIST_BASE[ds] + de
        else:
            length, dist = t
        assert 1 <= dist <= len(out), "distance before the start"
        for _ in range(length):
            out.append(out[-dist])
    return bytes(out[len(prefix):])


def _tokens(w, tokens, lit, dist, eob):
    for t in tokens:
        if isinstance(t, int):
            w.code(*lit[t])
            continue
        if t[0] == "sym":
            _, ls, le, ds, de = t
            lbits = LEN_EXTRA[ls - 257] if ls <= 285 else 0
            dbits = None if ds is None else (DIST_EXTRA[ds] if ds < 30 else 13)
        else:
            ls, lbits, le = length_symbol(t[0])
            ds, dbits, de = dist_symbol(t[1])
        assert lit[ls][1], "length symbol %d has no code" % ls
        w.code(*lit[ls])
        w.bits(le, lbits)
        if ds is not None:
            assert dist[ds][1], "distance symbol %d has no code" % ds
            w.code(*dist[ds])
            w.bits(de, dbits)
    if eob:
        assert lit[256][1], "no end-of-block code"
        w.code(*lit[256])


def stored(w, data, final=False, nlen=None):
    """A stored block (§3.2.4); nlen: the complement field as given (a mismatch when wrong)."""
    assert len(data) <= 65535
    w.bits(1 if final else 0, 1)
    w.bits(0, 2)
    w.align()
    w.bits(len(data), 16)
    w.bits((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
    for b in data:
        w.bits(b, 8)


def fixed(w, tokens, final=False, eob=True):
    """A block of the fixed codes (§3.2.6)."""
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    _tokens(w, tokens, canonical(FIXED_LIT), canonical(FIXED_DIST), eob)


def reserved(w, final=True):
    """The reserved block type 3."""
    w.bits(1 if final else 0, 1)
    w.bits(3, 2)


def cl_plain(lens):
    """Code lengths written one symbol each: [(symbol, extra value)]."""
    return [(l, 0) for l in lens]


def cl_rle(lens):
    """Code lengths with the repeat codes, greedily: zeros by 18 (11..138)
    and 17 (3..10), a repeated length by 16 (3..6 copies of the one before)."""
    out, i = [], 0
    while i < len(lens):
        j = i
        while j < len(lens) and lens[j] == lens[i]:
            j += 1
        r = j - i
        if lens[i] == 0:
            while r >= 11:
                k = min(r, 138)
                out.append((18, k - 11))
                r -= k
            if r >= 3:
                out.append((17, r - 3))
                r = 0
            out += [(0, 0)] * r
        else:
            out.append((lens[i], 0))
            r -= 1
            while r >= 3:
                k = min(r, 6)
                out.append((16, k - 3))
                r -= k
            out += [(lens[i], 0)] * r
        i = j
    return out


def cl_code_lengths(used):
    """A complete code of at most 7 bits over the code-length symbols `used`
    (a second symbol is added to a lone one: this code may not be incomplete)."""
    used = sorted(set(used))
    if len(used) == 1:
        used.append(0 if used[0] else 1)
    u = len(used)
    k = max(1, (u - 1).bit_length())
    short = (1 << k) - u
    lens = [0] * 19
    for i, s in enumerate(used):
        lens[s] = k - 1 if i < short else k
    return lens


def dynamic(w, tokens, lit_lens, dist_lens, final=False, eob=True, rle=False, cl_seq=None, cl_lens=None, ncode=None,
            nlen=None, ndist=None):
    """A block of dynamic codes (§3.2.7) with the given literal/length and
    distance code lengths (nlen / ndist: the header's counts, by default the
    lists' lengths).  The code lengths go out one symbol each, with the
    repeat codes (rle), or as cl_seq says ([(symbol, extra value)], over both
    lists as one, so a repeat may run from one into the other); cl_lens: the
    code-length code's own lengths (by default complete over the symbols
    used); ncode: how many of them are written (by default as few as hold
    them, at least 4)."""
    nlen = len(lit_lens) if nlen is None else nlen
    ndist = len(dist_lens) if ndist is None else ndist
    if cl_seq is None:
        cl_seq = (cl_rle if rle else cl_plain)(list(lit_lens) + list(dist_lens))
    if cl_lens is None:
        cl_lens = cl_code_lengths([s for s, _ in cl_seq])
    if ncode is None:
        ncode = max([4] + [i + 1 for i in range(19) if cl_lens[CL_ORDER[i]]])
    assert all(cl_lens[CL_ORDER[i]] == 0 for i in range(ncode, 19))
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits(nlen - 257, 5)
    w.bits(ndist - 1, 5)
    w.bits(ncode - 4, 4)
    for i in range(ncode):
        w.bits(cl_lens[CL_ORDER[i]], 3)
    cl = canonical(cl_lens)
    for s, e in cl_seq:
        assert cl[s][1], "code-length symbol %d has no code" % s
        w.code(*cl[s])
        w.bits(e, {16: 2, 17: 3, 18: 7}.get(s, 0))
    lit = canonical(list(lit_lens) + [0] * (288 - len(lit_lens)))
    dist = canonical(list(dist_lens) + [0] * (32 - len(dist_lens)))
    _tokens(w, tokens, lit, dist, eob)


def subfield(si, payload=b""):
    """A gzip extra subfield (RFC 1952 §2.3.1.1)."""
    assert len(si) == 2
    return si + struct.pack("<H", len(payload)) + payload


def bgzf_member(raw, data, before=b"", after=b"", crc=None, isize=None, cut=0):
    """A BGZF member around the raw DEFLATE bytes `raw`, which should inflate
    to `data`: extra subfields before / after the BC one (which holds BSIZE),
    crc / isize as given when not None (wrong ones on purpose), the last `cut`
    bytes of `raw` dropped (BSIZE follows, so the member chain stays whole)."""
    raw = raw[:len(raw) - cut] if cut else raw
    xlen = len(before) + 6 + len(after)
    bsize = 12 + xlen + len(raw) + 8 - 1
    assert bsize <= 65535, "a BGZF member holds at most 64 KiB of compressed bytes"
    crc = (zlib.crc32(data) & 0xFFFFFFFF) if crc is None else crc
    isize = len(data) if isize is None else isize
    return (struct.pack("<BBBBIBBH", 31, 139, 8, 4, 0, 0, 255, xlen) + before + b"BC" + struct.pack("<HH", 2, bsize) +
            after + raw + struct.pack("<II", crc, isize))


def layout(buf):
    """The members of a BGZF buffer, found as a reader must (the BC subfield
    among the extra subfields): [(src, csize, dst, isize)] -- the raw DEFLATE
    bytes at buf[src:src+csize], the output at [dst, dst+isize) of the
    inflated stream."""
    out, p, dst = [], 0, 0
    while p < len(buf):
        assert buf[p:p + 4] == b"\x1f\x8b\x08\x04"
        xlen, = struct.unpack_from("<H", buf, p + 10)
        q, bsize = p + 12, None
        while q < p + 12 + xlen:
            sl, = struct.unpack_from("<H", buf, q + 2)
            if buf[q:q + 2] == b"BC" and sl == 2:
                bsize, = struct.unpack_from("<H", buf, q + 4)
            q += 4 + sl
        assert q == p + 12 + xlen and bsize is not None
        isize, = struct.unpack_from("<I", buf, p + bsize + 1 - 4)
        out.append((p + 12 + xlen, bsize + 1 - 12 - xlen - 8, dst, isize))
        dst += isize
        p += bsize + 1
    assert p == len(buf)
    return out
