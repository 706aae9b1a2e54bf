"""Inputs for the realignment-target tests.

_pileup_gen places its reads at random over 90M positions, so no two share a
rod, and _mpileup_gen gives no control over quals.  Here a read is spelled
out -- ``read(pos0, cigar, md, ...)`` -- or cut from one hashed reference with
``overlapping``, a few thousand reads that overlap, carry indels, soft clips
and mismatches, and so yield every kind of target.  The header is
_pileup_gen's; records for the restatement come from ``_adam_ref.convert_sam``
over the very text the device parses."""
import random
import re

import _adam_ref
import _mpileup_gen as MG
import _pileup_gen as G

HEADER = G.HEADER
_EL = re.compile(r"([0-9]+)([MIDNSHP=X])")


def read_len(cigar: str) -> int:
    return sum(int(n) for n, op in _EL.findall(cigar) if op in "MIS=X")


def read(pos0, cigar, md, seq=None, qual=None, flag=16, rname="c1", name=None):
    """One SAM line's fields; seq and qual default to "A" * length, as
    IndelRealignmentTargetSuite.make_read has them (md None: no MD tag)"""
    n = read_len(cigar)
    seq = "A" * n if seq is None else seq
    return dict(pos0=pos0, cigar=cigar, md=md, seq=seq or "*", qual=(seq if qual is None else qual) or "*", flag=flag,
                rname=rname, name=name)


def sam_text(reads) -> bytes:
    lines = []
    for i, r in enumerate(reads):
        tags = [] if r["md"] is None else [b"MD:Z:" + r["md"].encode()]
        lines.append(b"\t".join([(r["name"] or "read%d" % i).encode(), b"%d" % r["flag"], r["rname"].encode(),
                                 b"%d" % (r["pos0"] + 1), b"60", r["cigar"].encode(), b"*", b"0", b"0",
                                 r["seq"].encode(), r["qual"].encode("latin-1")] + tags) + b"\n")
    return HEADER + b"".join(lines)


def records(text: bytes):
    return _adam_ref.convert_sam(text, G.run_date)


CIGARS = ("50M", "50M", "50M", "20M2D30M", "25M1I24M", "10M3I37M", "3S47M", "45M5S", "20M1D10M2I18M", "30M4D20M",
          "50M", "12M2D38M")


def overlapping(n=3000, seed=11, span=40000):
    """n reads of 50 bases cut from _mpileup_gen's hashed reference of c1 (a
    tenth on c2, at the same positions: shared rods), sorted by nothing in
    particular, dense enough that rods are a few reads deep; a few islands of
    reads stand alone, so that single-rod targets exist too"""
    rnd = random.Random(seed)
    out = []
    for i in range(n):
        rname = "c2" if i % 10 == 9 else "c1"
        pos0 = rnd.randrange(1000, 1000 + span)
        cigar = rnd.choice(CIGARS)
        seq, md = MG.read_fields(rnd, rname, pos0, cigar, mismatch=rnd.choice((0.0, 0.0, 0.02, 0.3)))
        qual = G._quals(rnd, len(seq), wide=False).decode("latin-1")
        out.append(read(pos0, cigar, md, seq=seq, qual=qual, flag=rnd.choice((0x10, 0x1 | 0x40, 0x1 | 0x80 | 0x10)),
                        rname=rname))
    # islands: one read with exactly one piece of evidence, far from everything
    for k, (cigar, md) in enumerate((("5M1I5M", "10"), ("5M2D5M", "5^AC5"), ("2S8M", "8"), ("10M", "4C5"))):
        out.append(read(10_000_000 + 1000 * k, cigar, md, seq="G" * read_len(cigar), qual="I" * read_len(cigar)))
    # two reads with differing starts and the same 1-base insertion, alone: a single rod, two ranges
    out.append(read(20_000_000, "6M1I6M", "12", seq="G" * 13, qual="I" * 13))
    out.append(read(20_000_002, "4M1I6M", "10", seq="G" * 11, qual="I" * 11))
    rnd.shuffle(out)
    return out
