"""The crafted BGZF members of test_gpu_bgzf_bytes.py, by group (a group is
one BGZF buffer, one bqsr_bgzf_inflate call).  test_deflate_writer.py holds
every one of them against zlib on the CPU: a member with ``good`` set must
inflate (``zlib.decompress(raw, -15)``) to ``data`` and pass as a gzip member
(CRC32, ISIZE); every other must raise ``zlib.error`` as a gzip member.

Two limits of the container shape the cases.  A BGZF member is at most
64 KiB of compressed bytes (BSIZE is 16 bits), so its largest stored block
is 65505 bytes, not 65535.  And no valid DEFLATE stream is shorter than two
bytes (an empty fixed block is 10 bits), nor has a valid dynamic block fewer
than 5 code-length code lengths (the first four are 16, 17, 18 and 0: with
only those every length is 0 and there is no end-of-block code): the 1-byte
stream and the ncode-4 block are among the malformed members.
"""
import zlib

import _deflate as D


class Member:
    def __init__(self, name, raw, data, good=True, **wrap):
        self.name, self.raw, self.data, self.good, self.wrap = name, raw, data, good, wrap

    def bytes(self):
        return D.bgzf_member(self.raw, self.data, **self.wrap)


class Stream:
    """A DEFLATE stream built block by block, with the bytes it stands for."""

    def __init__(self):
        self.w = D.BitWriter()
        self.out = b""

    def stored(self, data, final=False, **kw):
        D.stored(self.w, data, final, **kw)
        self.out += bytes(data)
        return self

    def fixed(self, tokens, final=False, **kw):
        D.fixed(self.w, tokens, final, **kw)
        self.out += D.expand(tokens, self.out)
        return self

    def dynamic(self, tokens, lit_lens, dist_lens, final=False, **kw):
        D.dynamic(self.w, tokens, lit_lens, dist_lens, final, **kw)
        self.out += D.expand(tokens, self.out)
        return self

    def member(self, name, good=True, **wrap):
        return Member(name, self.w.bytes(), self.out, good, **wrap)


def flat_lengths(used, size):
    """Code lengths over `size` symbols, complete over the symbols `used` (a lone one: length 1)."""
    used = sorted(set(used))
    lens = [0] * size
    if len(used) == 1:
        lens[used[0]] = 1
        return lens
    k = (len(used) - 1).bit_length()
    short = (1 << k) - len(used)
    for i, s in enumerate(used):
        lens[s] = k - 1 if i < short else k
    return lens


def lens_for(tokens, nlen=None, ndist=None):
    """Flat complete codes over exactly the symbols a token list uses (and end-of-block)."""
    ls, ds = {256}, set()
    for t in tokens:
        if isinstance(t, int):
            ls.add(t)
        elif t[0] == "sym":
            ls.add(t[1])
            if t[3] is not None:
                ds.add(t[3])
        else:
            ls.add(D.length_symbol(t[0])[0])
            ds.add(D.dist_symbol(t[1])[0])
    nlen = max(257, max(ls) + 1) if nlen is None else nlen
    ndist = (max(ds) + 1 if ds else 1) if ndist is None else ndist
    return flat_lengths(ls, nlen), (flat_lengths(ds, ndist) if ds else [0] * ndist)


def second_level_widths(lengths, root):
    """The index widths of a canonical code's second-level decode tables (one per root prefix of longer codes)."""
    widths, prev = [], None
    for (c, l) in sorted((x for x in D.canonical(lengths) if x[1] > root), key=lambda x: x[0] << (15 - x[1])):
        g = c >> (l - root)
        if g != prev:
            widths.append(0)
            prev = g
        widths[-1] = max(widths[-1], l - root)
    return widths


def use_all(lit_lens, dist_lens, limit=65536, lead=2):
    """Tokens that use every code of a pair of codes: every literal (`lead`
    times over), every length symbol and every distance symbol each at its
    smallest and largest extra-bit value, a literal after every other match."""
    lits = [s for s in range(256) if lit_lens[s]]
    lsyms = [s for s in range(257, min(286, len(lit_lens))) if lit_lens[s]]
    dsyms = [s for s in range(min(30, len(dist_lens))) if dist_lens[s]]
    toks = (lits + lits[::-1]) * lead
    toks = toks[:len(lits) * lead]
    pos = len(toks)
    if not lsyms or not dsyms:
        return toks
    assert pos > 0
    pl = [(s, e) for s in lsyms for e in sorted({0, (1 << D.LEN_EXTRA[s - 257]) - 1})]
    pd = [(s, e) for s in dsyms for e in sorted({0, (1 << D.DIST_EXTRA[s]) - 1})]
    i = 0
    while pd or i < len(pl):
        ls, le = pl[i % len(pl)]
        if pd and D.DIST_BASE[pd[0][0]] + pd[0][1] <= pos:
            ds, de = pd.pop(0)
        else:
            ds, de = dsyms[0], 0
            assert D.DIST_BASE[ds] <= pos
        toks.append(("sym", ls, le, ds, de))
        pos += D.LEN_BASE[ls - 257] + le
        if i & 1:
            toks.append(lits[i % len(lits)])
            pos += 1
        i += 1
        assert pos <= limit, "use_all: the codes' symbols do not fit the limit"
    return toks


def dyn(name, tokens, lit_lens, dist_lens, good=True, wrap=None, **kw):
    s = Stream().dynamic(tokens, lit_lens, dist_lens, final=True, **kw)
    return s.member(name, good, **(wrap or {}))


def fix(name, tokens, good=True, **wrap):
    return Stream().fixed(tokens, final=True).member(name, good, **wrap)


def text(n, seed=1):
    """n compressible bytes (SAM-like: few symbols, repeats at many distances)."""
    out, x = bytearray(), seed
    while len(out) < n:
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        if (x >> 8) % 3 == 0 and len(out) > 8:
            d = 1 + (x >> 12) % min(len(out), 40000)
            k = 3 + (x >> 4) % 70
            for _ in range(k):
                out.append(out[-d])
        else:
            out += b"ACGT#IJ\t0123456789"[(x >> 5) % 18:][:1 + (x >> 9) % 5]
    return bytes(out[:n])


def lz_tokens(data):
    """A greedy LZ77 parse of `data` (the longest earlier occurrence, found by its first three bytes)."""
    toks, i = [], 0
    while i < len(data):
        j = data.rfind(data[i:i + 3], 0, i + 2) if i + 3 <= len(data) else -1
        if j < 0 or j >= i:
            toks.append(data[i])
            i += 1
            continue
        n = 3
        while n < 258 and i + n < len(data) and data[j + n] == data[i + n]:
            n += 1
        toks.append((n, i - j))
        i += n
    return toks


def zlib_member(name, data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, **wrap):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return Member(name, c.compress(data) + c.flush(), data, True, **wrap)


# ---- literal / length and distance codes --------------------------------

# a complete literal/length code whose longer codes fall, in code order, into
# six root-9 prefixes holding codes of at most 10, 11, 12, 13, 14, 15 bits
LIT15_SORTED = [1, 2, 3, 4, 5, 6, 8] + [10] * 3 + [11] * 4 + [12] * 8 + [13] * 16 + [14] * 32 + [15] * 32
# (the short codes -- root-table entries -- to end-of-block, four literals and two length symbols)
LIT15_SYMS = [256, 65, 66, 67, 257, 258, 68] + list(range(259, 268)) + [s for s in range(90) if not 65 <= s <= 68]
LIT15 = [0] * 268
for _s, _l in zip(LIT15_SYMS, LIT15_SORTED):
    LIT15[_s] = _l
# distance codes with 9- to 15-bit members
DIST15 = list(range(1, 16)) + [15]
# 30 distance codes (a complete code, 9- to 15-bit members in three root-8 prefixes)
DIST30 = [1, 2, 3, 4, 5, 6, 8] + [9, 10, 11, 12, 13, 14, 15, 15] * 2 + [9, 10, 11, 12, 13, 14, 14]
FIXED286 = D.FIXED_LIT[:286]
# a complete code over all 286 symbols: the fixed code without 286 and 287, four 9-bit codes made 8-bit
LIT286 = [8 if 144 <= s < 148 else l for s, l in enumerate(FIXED286)]

# code lengths whose greedy run-length form uses 16, 17 and 18 each at its
# smallest and largest count, and a 16 that runs from the literal/length
# lengths into the distance lengths
RLE_LIT = ([4] * 4 + [0] * 3 + [4] * 7 + [0] * 10 + [4] + [0] * 11 + [4] + [0] * 138 + [0] * 80 + [5, 5, 4, 4])
RLE_DIST = [4, 4, 4, 4, 2, 1]
RLE_WANT = [(16, 0), (17, 0), (16, 3), (17, 7), (18, 0), (18, 127), (18, 80 - 11), (16, 2)]


def group_codes():
    m = []
    m.append(dyn("lit15-dist15", use_all(LIT15, DIST15), LIT15, DIST15))
    m.append(dyn("lit15-dist15-rle", use_all(LIT15, DIST15), LIT15, DIST15, rle=True))
    m.append(fix("fixed-every-symbol", use_all(FIXED286, D.FIXED_DIST[:30], lead=1)))
    m.append(dyn("nlen286-ndist30", use_all(LIT286, DIST30, lead=1), LIT286, DIST30, rle=True))
    m.append(fix("len258-by-284", [7, ("sym", 284, 31, 0, 0), ("sym", 284, 30, 0, 0), ("sym", 285, 0, 0, 0)]))
    t = [1, 2, 3, (3, 3), (6, 6), 9, (13, 13), (258, 26)]
    m.append(fix("dist-eq-pos-fixed", t))
    m.append(dyn("dist-eq-pos-dynamic", t, *lens_for(t)))
    t = [5, (258, 1), (17, 1)]
    m.append(dyn("lone-dist-code-0", t, *lens_for(t)))
    t = [5, 6, 7, 8, 9, (4, 5), (30, 6)]
    m.append(dyn("lone-dist-code-4", t, *lens_for(t)))
    t = list(b"no distance code at all") * 3
    m.append(dyn("no-dist-code", t, *lens_for(t)))
    m.append(dyn("lone-eob", [], [0] * 256 + [1], [0]))
    m.append(Stream().dynamic([], [0] * 256 + [1], [0]).fixed(t).dynamic([], [0] * 256 + [1], [0], final=True)
             .member("lone-eob-blocks"))
    m.append(dyn("cl-repeats", use_all(RLE_LIT, RLE_DIST), RLE_LIT, RLE_DIST, rle=True))
    # ncode: 5 is the fewest a valid block has (lengths 0 and 8 only: 256 codes of 8 bits); 19 with trailing zeros,
    # and with the last one (length 15) in use
    l8 = [8] * 255 + [0, 8]
    m.append(dyn("ncode5", list(range(255)), l8, [0]))
    m.append(dyn("ncode19-zeros", list(range(255)), l8, [0], ncode=19))
    m.append(dyn("ncode19-len15", use_all(LIT15, DIST15), LIT15, DIST15, ncode=19))
    t = [0, 255, 0]
    m.append(dyn("nlen257-ndist1", t, *lens_for(t)))
    return m


# ---- block structure -----------------------------------------------------

def group_blocks():
    m = []
    a, b, c = b"stored bytes, ", list(b"fixed codes, "), list(b"dynamic ones; ")
    back = [(9, 14), (20, 30)]
    dl = lens_for(c + back)
    kinds = {"s": lambda s, f: s.stored(a, f), "f": lambda s, f: s.fixed(b + (back if len(s.out) >= 30 else []), f),
             "d": lambda s, f: s.dynamic(c + (back if len(s.out) >= 30 else []), dl[0], dl[1], f)}
    for order in ("sfd", "sdf", "fsd", "fds", "dsf", "dfs"):
        s = Stream()
        for i, k in enumerate(order * 2):
            kinds[k](s, i == 5)
        m.append(s.member("mixed-" + order))
    m.append(Stream().fixed(b).stored(b"").fixed(b + back, True).member("empty-stored-mid"))
    for flush in (zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH):
        z = zlib.compressobj(6, zlib.DEFLATED, -15)
        data = text(3000, 5)
        raw = z.compress(data[:1000]) + z.flush(flush) + z.compress(data[1000:]) + z.flush()
        m.append(Member("zlib-flush-%d" % flush, raw, data))
    for j in range(8):  # a stored block whose header ends at each bit offset (j 9-bit literals before it)
        m.append(Stream().fixed([200] * j + [65]).stored(b"at a bit offset", True).member("stored-bit-%d" % j))
    m.append(Stream().stored(b"", True).member("stored-0"))
    m.append(Stream().stored(text(65505, 9), True).member("stored-65505"))
    m.append(Stream().stored(a).fixed([], True).member("final-empty-fixed"))
    m.append(Stream().fixed(b).stored(b"", True).member("final-empty-stored"))
    m.append(Stream().fixed(b).dynamic([], [0] * 256 + [1], [0], True).member("final-empty-dynamic"))
    # the second literal of a step: the block's last before end-of-block (the member's last byte), in the root
    # table (8 and 9 bits) and not (LIT15's literals of 10 to 15 bits after one of 8)
    m.append(fix("two-literals", [65, 66]))
    m.append(fix("two-literals-9bit", [65, 200]))
    m.append(fix("three-literals", [65, 66, 67]))
    m.append(fix("match-then-literal", [65, (5, 1), 66]))
    m.append(Stream().fixed([65, 66]).fixed([67, 68], True).member("two-literals-two-blocks"))
    long_lits = [s for s in range(90) if LIT15[s] > 9]
    t = [x for s in long_lits for x in (68, s)] + [65, (3, 2), long_lits[-1]]
    m.append(dyn("literal-then-second-level", t, LIT15, DIST15))
    return m


def stored_bit_offsets():
    """(the bit offset at which each stored-bit-j member's stored header ends)"""
    out = []
    for j in range(8):
        w = D.BitWriter()
        D.fixed(w, [200] * j + [65])
        out.append((w.bitpos + 3) % 8)
    return out


# ---- the bit reader --------------------------------------------------------

def sized(n, seed):
    """A fixed-codes member of exactly n compressed bytes (n >= 2): matches and literals, 8-bit literals to fill."""
    toks = []
    if n > 40:
        toks = list(b"ring wrap ") + [(4 + (seed + i) % 30, 1 + (i * 7 + seed) % 10) for i in range((n - 30) // 3)]
    while True:
        w = D.BitWriter()
        D.fixed(w, toks, True)
        if len(w.bytes()) >= n:
            break
        toks.append(97 + len(toks) % 26)
    assert len(w.bytes()) == n, (n, len(w.bytes()))
    return fix("csize-%d" % n, toks)


CSIZES = [2, 127, 128, 129, 255, 256, 257, 600]


def group_reader():
    m = []
    base = use_all(LIT15, DIST15)
    off = 0
    for k in range(16):  # the same member at every start alignment mod 16, by an extra subfield before BC of 4 to 19 bytes
        mm = dyn("align-%d" % k, base, LIT15, DIST15)
        after = D.subfield(b"ZZ", b"after") if k & 1 else b""
        mm.wrap = {"before": D.subfield(b"AL", bytes((k - (off + 12 + 4 + 6 + len(after))) % 16)), "after": after}
        off += len(mm.bytes())
        m.append(mm)
    m += [sized(n, n) for n in CSIZES]
    m.append(Member("csize-1-reserved", b"\x07", b"", False))
    m.append(Member("csize-0", b"", b"", False))
    m.append(fix("ends-on-a-byte", [200] * 6))
    m.append(zlib_member("zlib-text", text(20000, 3)))
    m.append(fix("ends-on-a-byte-last", [65, 200, 201, 202, 203, 204, 205]))  # (the buffer's last member: no EOF block)
    return m


# ---- the resolve pass, ISIZE, CRC32 -----------------------------------------

TOKEN_COUNTS = [0, 1, 511, 512, 513, 1024, 1025]
ISIZES = [0, 1, 2, 3, 4, 5, 131, 132, 133, 263, 264, 65535, 65536]
SMALL = [s for s in ISIZES if s < 1000]


def n_tokens(n):
    toks = []
    for i in range(n):
        toks.append((3 + i % 9, 1 + i % min(len(toks), 33)) if i % 3 == 2 else 32 + i % 90)
    return toks


def group_resolve():
    m = [fix("tokens-%d" % n, n_tokens(n)) for n in TOKEN_COUNTS]
    lit = [32 + i % 95 for i in range(512)]
    m.append(fix("group-first-match", lit + [(10, 512), (8, 5), (258, 300)]))
    m.append(fix("group-first-match-2", lit + [(3, 1)] + lit[:511] + [(258, 1023), 7]))
    m.append(fix("chain-512-in-one-group", lit[:509] + [1, 2, 3] + [(3, 3)] * 512))
    m.append(fix("chain-512", [1, 2, 3] + [(3, 3)] * 512))
    t = list(range(100, 109))
    for d in range(1, 10):
        for n in (3, 7, 8, 9, 16, 17, 258):
            t += [(n, d), 50 + d]
    m.append(fix("dist-1-9", t))
    t = list(range(100, 112))
    for d in range(1, 10):  # (and the same at every output alignment mod 8)
        for n in (8, 9, 16, 17):
            t += [(n, d)] + [60] * (d % 3)
    m.append(dyn("dist-1-9-dynamic", t, *lens_for(t)))
    return m


def isize_member(n, seed=0):
    if n < 1000:
        return fix("isize-%d" % n, [(40 + 7 * i + seed) % 251 for i in range(n)])
    return zlib_member("isize-%d" % n, text(n, n + seed))


def group_isize():
    """A correct member of every ISIZE; the small ones at every output alignment mod 4 (members of 0 to 3 bytes before them)."""
    m = [isize_member(n) for n in ISIZES]
    dst = sum(ISIZES)
    for n in SMALL:
        for a in range(4):
            pad = (a - dst) % 4
            m.append(isize_member(pad, 3))
            m.append(isize_member(n, a))
            dst += pad + n
    return m


# ---- malformed members --------------------------------------------------------

def group_invalid():
    """Members the decoder must decline, a good one before and after each."""
    bad = []
    add = bad.append
    add(Member("type-3", _with(lambda w: (D.fixed(w, [65]), D.reserved(w))), b"A", False))
    add(Stream().stored(b"len and nlen differ", True, nlen=0x1234).member("stored-nlen", False))
    t = [65, 66, 67, (3, 2)]
    ll, dl = lens_for(t)
    add(dyn("nlen-287", t, ll + [0] * (287 - len(ll)), dl, False))
    add(dyn("ndist-31", t, ll, dl + [0] * (31 - len(dl)), False))
    over = list(ll)
    over[68] = 1
    add(dyn("lit-oversubscribed", t, over, dl, False))
    add(dyn("dist-oversubscribed", t, ll, [1, 1, 1], False))
    add(dyn("lit-incomplete-two-symbols", [65], _at([0] * 257, {65: 2, 256: 2}), [0], False))
    add(dyn("lit-incomplete-three-symbols", [65, 66], _at([0] * 257, {65: 2, 66: 2, 256: 2}), [0], False))
    add(dyn("dist-incomplete-two-symbols", [65, 66, 67, (3, 2), (3, 1)], ll, [2, 2], False))
    noeob = _at([0] * 258, {65: 1, 257: 1})
    add(dyn("no-eob-code", [65], noeob, [1], False, eob=False))
    add(dyn("cl-16-first", [], _at([0] * 257, {0: 1, 256: 1}), [0], False,
            cl_seq=[(16, 0)] + [(1, 0)] + [(0, 0)] * 251 + [(1, 0), (0, 0)], cl_lens=_at([0] * 19, {0: 1, 1: 2, 16: 2})))
    add(dyn("cl-repeat-past-end", [65], _at([0] * 257, {65: 1, 256: 1}), [0], False,
            cl_seq=[(18, 65 - 11), (1, 0), (18, 127), (18, 256 - 66 - 138 - 11), (1, 0), (17, 0)]))
    add(dyn("ncode-4", [], [0] * 257, [0], False, eob=False, cl_seq=[(18, 127), (18, 120 - 11)],
            cl_lens=_at([0] * 19, {18: 1, 0: 1}), ncode=4))
    for ls in (286, 287):
        add(Member("fixed-len-%d" % ls, _with(lambda w, ls=ls: D.fixed(w, [65, 66, 67, ("sym", ls, 0, None, 0)], True)),
                   b"ABC", False))
    for ds in (30, 31):
        add(Member("fixed-dist-%d" % ds, _with(lambda w, ds=ds: D.fixed(w, [65, 66, 67, ("sym", 257, 0, ds, 0)], True)),
                   b"ABCABC", False))
    add(Member("dist-gt-pos", _with(lambda w: D.fixed(w, [65, 66, ("sym", 257, 0, 2, 0)], True)), b"AB" + b"ABA", False))
    add(Member("dist-gt-pos-0", _with(lambda w: D.fixed(w, [("sym", 257, 0, 0, 0)], True)), b"AAA", False))
    add(fix("over-isize-literal", [65, 66, 67], False, isize=2))
    add(fix("over-isize-second-literal", [65, 66], False, isize=1))
    add(fix("over-isize-match", [65, (5, 1)], False, isize=5))
    add(Stream().stored(b"stored", True).member("over-isize-stored", False, isize=5))
    add(fix("short-of-isize", [65, (5, 1)], False, isize=7))
    add(fix("short-of-isize-empty", [], False, isize=1))
    add(zlib_member("cut-1", text(5000, 7)))
    bad[-1].good, bad[-1].wrap = False, {"cut": 1}
    add(zlib_member("cut-8", text(5000, 8)))
    bad[-1].good, bad[-1].wrap = False, {"cut": 8}
    add(Stream().stored(b"a stored block cut short", True).member("cut-1-stored", False, cut=1))
    add(dyn("lone-lit-code-length-5", [], _at([0] * 257, {256: 5}), [0], False))
    add(dyn("lone-lit-code-length-2", [], _at([0] * 257, {256: 2}), [0], False))
    t = [65, 66, 67, 68, (4, 1), (3, 1)]
    add(dyn("lone-dist-code-length-3", t, lens_for(t)[0], [3], False))
    t = [65, 66, 67, 68, (4, 3), (3, 3)]
    add(dyn("lone-dist-code-length-15", t, lens_for(t)[0], [0, 0, 15], False))
    good = zlib_member("crc-good", text(700, 2))
    add(Member("crc-bit", good.raw, good.data, False, crc=(zlib.crc32(good.data) ^ 0x00010000) & 0xFFFFFFFF))
    d = bytearray(text(300, 4))
    raw = bytearray(Stream().stored(bytes(d), True).w.bytes())
    raw[5 + 150] ^= 0x08
    add(Member("data-bit", bytes(raw), bytes(d), False))
    m = []
    for i, b in enumerate(bad):
        m.append(isize_member(1 + i % 7, i) if i % 3 else zlib_member("good-%d" % i, text(900 + i, i)))
        m.append(b)
    m.append(zlib_member("good-last", text(1234, 11)))
    return m


def _with(f):
    w = D.BitWriter()
    f(w)
    return w.bytes()


def _at(lens, at):
    lens = list(lens)
    for s, l in at.items():
        lens[s] = l
    return lens


GROUPS = {"codes": group_codes, "blocks": group_blocks, "reader": group_reader, "resolve": group_resolve,
          "isize": group_isize, "invalid": group_invalid}


def pack(members, eof=False):
    buf = b"".join(m.bytes() for m in members)
    if eof:
        buf += D.bgzf_member(b"\x03\x00", b"")
    return buf
