"""Generated reads for the mpileup tests.  `adam mpileup` merges the events of
all reads at a position and the reference asserts that they agree on the
reference base, so -- unlike the reads of _pileup_gen, each with a reference
of its own -- these reads are cut from ONE reference per contig (a hash of
the position, so any position exists) and carry sequence and MD consistent
with it.  The MD text itself, the quals and the header are _pileup_gen's.

A read is given as (pos0, cigar[, options]): its 0-based start, its CIGAR
text, and optionally flag, rname, mapq, mismatch rate, or ready-made seq /
md.  The MD offset is referencePos - start the way the reference reads it:
N, = and X spans count as matches."""
import random
import re

import _adam_ref
import _pileup_gen as G

HEADER = G.HEADER
_EL = re.compile(r"([0-9]+)([MIDNSHP=X])")


def ref_base(contig: str, pos: int) -> str:
    x = (pos * 2654435761 + sum(contig.encode()) * 40503) & 0xFFFFFFFF
    x = ((x ^ (x >> 13)) * 0x5BD1E995) & 0xFFFFFFFF
    x ^= x >> 15
    return "ACGT"[x & 3] if (x >> 2) % 16 else "N"


def read_fields(rnd, contig, pos0, cigar, mismatch=0.1):
    """(sequence, MD text) of a read at pos0 with this CIGAR, cut from the contig's reference"""
    seq, kinds, pos = [], [], pos0
    for k, op in ((int(a), b) for a, b in _EL.findall(cigar)):
        if op == "M":
            for _ in range(k):
                r = ref_base(contig, pos)
                if rnd.random() < mismatch:
                    seq.append(rnd.choice([b for b in "ACGTN" if b != r]))
                    kinds.append(("X", r))
                else:
                    seq.append(r)
                    kinds.append(None)
                pos += 1
        elif op == "D":
            for _ in range(k):
                kinds.append(("D", ref_base(contig, pos)))
                pos += 1
        elif op in "IS":
            seq += [rnd.choice("ACGTN") for _ in range(k)]
        elif op in "N=X":
            if op != "N":
                seq += [rnd.choice("ACGT") for _ in range(k)]
            kinds += [None] * k
            pos += k
    return "".join(seq) or "*", G.md_of(rnd, kinds)


def sam_text(specs, seed=1):
    """SAM text (HEADER + one line per spec, in the order given)"""
    rnd = random.Random(seed)
    lines = []
    for i, spec in enumerate(specs):
        pos0, cigar = spec[0], spec[1]
        o = dict(spec[2]) if len(spec) > 2 else {}
        rname = o.get("rname", "c1")
        flag = o.get("flag", rnd.choice((16, 1 | 64, 1 | 128 | 16, 1 | 2 | 32, 2048, 32)))
        seq, md = ("ACGT", None) if cigar == "*" else read_fields(rnd, rname, pos0, cigar, o.get("mismatch", 0.1))
        seq = o.get("seq", seq)
        md = o.get("md", md)
        qual = G._quals(rnd, len(seq), wide=False) if seq != "*" else b"*"
        tags = [] if md is None else [b"MD:Z:" + md.encode()]
        if rnd.randrange(2):
            tags.append(b"NM:i:%d" % rnd.randrange(5))
        lines.append(b"\t".join([b"r%d" % i, b"%d" % flag, rname.encode(), b"%d" % (pos0 + 1),
                                 b"%d" % o.get("mapq", rnd.choice((0, 7, 30, 60))), cigar.encode(), b"*", b"0", b"0",
                                 seq.encode(), qual] + tags) + b"\n")
    return HEADER + b"".join(lines)


def records(text):
    return _adam_ref.convert_sam(text, G.run_date)
