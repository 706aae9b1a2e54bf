"""Coordinate-sorted SAM texts for the .bai tests: each shape at the smallest
size at which the index can still go wrong.  ``SHAPES`` maps a name to a
function that returns the text; ``REGIONS`` are the (refID, beg, end) queries
every shape is read back with."""
from __future__ import annotations

from typing import Callable, Dict, List

HEAD = (b"@HD\tVN:1.4\tSO:coordinate\n@SQ\tSN:chr1\tLN:536870912\n@SQ\tSN:chr2\tLN:1000000\n"
        b"@SQ\tSN:chr3\tLN:536870912\n@RG\tID:g1\tLB:l1\tSM:s\n")
B14, B17, B20, B23, B26 = 7 << 14, 3 << 17, 3 << 20, 3 << 23, 1 << 26  # multiples of one level and not of the next


def rec(qname: bytes, flag: int, rname: bytes, pos: int, cigar: bytes, seq: bytes, qual: bytes = None) -> bytes:
    return b"\t".join([qname, b"%d" % flag, rname, b"%d" % pos, b"30", cigar, b"*", b"0", b"0", seq,
                       qual if qual is not None else b"I" * len(seq)]) + b"\n"


def short(qname: bytes, rname: bytes, pos: int, flag: int = 0, cigar: bytes = b"30M") -> bytes:
    return rec(qname, flag, rname, pos, cigar, b"ACGTTGCAACGTTGCAACGTTGCAACGTTG")


def long_reads(n: int = 300) -> bytes:
    """SEQ near 4000 bases: about ten records a member, records that straddle two"""
    out = [HEAD]
    for i in range(n):
        L = 3990 + (i * 7) % 21
        out.append(rec(b"L%d" % i, 0, b"chr1", 100001 + 53 * i, b"%dM" % L, (b"ACGT" * 1004)[i % 4:][:L]))
    return b"".join(out)


def exact_member(tail: int) -> bytes:
    """the first record is 65280 bytes of BAM (36 + "A\\0" + one CIGAR word +
    21746 + 43492): it ends exactly on the first member boundary of its piece;
    tail = 0: it is the last record and the stream ends there"""
    L = 43492
    out = [HEAD, rec(b"A", 0, b"chr1", 1000, b"%dM" % L, b"ACGT" * (L // 4))]
    out += [short(b"t%d" % i, b"chr1", 2000 + i) for i in range(tail)]
    return b"".join(out)


def bins_and_windows() -> bytes:
    """the first read at 100 000 (leading windows hold 0); N operators across a
    boundary of every level (the 2^26 one: bin 0); a read over five windows;
    gaps above 16 kb"""
    out = [HEAD, short(b"first", b"chr1", 100001)]
    for k, b in enumerate((B14, B17, 500000 - 40, B20, B23, B26)):
        if b == 500000 - 40:
            out.append(rec(b"five", 0, b"chr1", 500001, b"10M65536N10M", b"ACGTACGTACGTACGTACGT"))
            continue
        out.append(short(b"in%d" % k, b"chr1", b - 200))                      # ends before the boundary
        out.append(rec(b"x%d" % k, 0, b"chr1", b - 99, b"50M200N50M", b"ACGT" * 25))  # crosses it
        out.append(short(b"at%d" % k, b"chr1", b + 1))                        # starts on it
    out.append(short(b"c3", b"chr3", 1 << 20))
    return b"".join(out)


def chunk_runs() -> bytes:
    """leaf bins of 65, 257 and 1025 consecutive records; then, just below
    2^26, records of a leaf bin alternating with records of bin 0 (an N across
    2^26) in runs of 5 (far shorter than a member's ~690 records) and of 1500
    (longer than two members)"""
    out = [HEAD]
    k = 0
    for w, n in ((10, 65), (20, 257), (30, 1025)):
        for i in range(n):
            out.append(short(b"b%d" % k, b"chr1", (w << 14) + 1 + 3 * i))
            k += 1
    pos = B26 - 16000
    for run in (5, 5, 5, 5, 1500, 1500, 5, 5, 1500, 5):
        for zero in (False, True):
            for _ in range(run):
                out.append(short(b"z%d" % k, b"chr1", pos, cigar=b"15M20000N15M") if zero
                           else short(b"l%d" % k, b"chr1", pos))
                k += 1
                pos += 1
    return b"".join(out)


def references() -> bytes:
    """reads on the first and the third of three references, a read with an
    RNAME and POS 0, a placed read with FLAG 0x4, unplaced reads at the end"""
    out = [HEAD, rec(b"pos0", 0, b"chr1", 0, b"*", b"ACGT"), short(b"a", b"chr1", 5000),
           short(b"un_placed", b"chr1", 5000, flag=4, cigar=b"*"), short(b"b", b"chr1", 40000, flag=16),
           short(b"c", b"chr3", 7), short(b"d", b"chr3", 70000, flag=0x404)]
    out += [rec(b"u%d" % i, 4, b"*", 0, b"*", b"ACGTA") for i in range(3)]
    return b"".join(out)


def header_only() -> bytes:
    return HEAD


SHAPES: Dict[str, Callable[[], bytes]] = {
    "long_reads": long_reads,
    "exact_member_then_more": lambda: exact_member(70),
    "exact_member_last": lambda: exact_member(0),
    "bins_and_windows": bins_and_windows,
    "chunk_runs": chunk_runs,
    "references": references,
    "header_only": header_only,
}

REGIONS: List[tuple] = [
    (0, 0, 50000),                    # before the first read of most shapes
    (0, 200000, 210000),              # inside an empty window of bins_and_windows
    (0, B14 - 10, B14 + 10), (0, B17 - 10, B17 + 10), (0, B26 - 10, B26 + 10),
    (0, B26 - 16000, B26 - 15990),
    (0, 500000, 500001), (0, 540000, 540001),
    (0, 0, 1 << 29),                  # a whole reference
    (1, 0, 1 << 29),                  # a reference without reads
    (2, 0, 1 << 29),
]


def lines(text: bytes) -> List[bytes]:
    return [l + b"\n" for l in text.split(b"\n") if l and not l.startswith(b"@")]


def sort_text(text: bytes) -> bytes:
    """a SAM text's records in (@SQ index, POS) order, unplaced ones last, ties in input order"""
    head = [l + b"\n" for l in text.split(b"\n") if l.startswith(b"@")]
    names = [f.split(b"\t")[1][3:] for f in head if f.startswith(b"@SQ")]
    idx = {n: i for i, n in enumerate(names)}

    def key(l):
        f = l.split(b"\t")
        return (idx.get(f[2], len(names)), int(f[3]) if f[2] in idx else 0)
    return b"".join(head + sorted(lines(text), key=key))
