"""Inputs that drive the expectedMismatch fold (adam_amd/csrc/bqsr_fold.hip)
through each of its paths, and a plain sequential reference of the fold.

The fold replays ``expectedMismatch += pow10cache[q]`` over a partition's
folded bases bit for bit without adding in order: inside a binade
[2^e, 2^(e+1)) an addition is an exact integer increment of round(t / u) units
u = 2^(e-52), except where t / u is exactly a half-integer (a tie), where the
sum leaves the binade (a crossing), and while S < 1/16 (one addition at a
time).  ``ref_fold`` performs the additions one by one in IEEE double and
reports where those events are, so that a test can tell that an input demands
the path it was built for; the builders below produce such inputs.

Where a qual can tie follows from the bits of t = 10^(-q/10): t = M * 2^(et-52)
with a 53-bit integer M, so t / u = M * 2^(et-e) is a half-integer at exactly
one binade, e = et + 1 + (trailing zeros of M) -- ``TIE_BINADE``.  For
q = 1..127 that binade is at most 4: no addition ties once S >= 32.  (q = 0,
t = 1, ties at e = 53 only.)

Every path of the fold is reached by one of the cases (DESIGN.md lists which).
"""
from __future__ import annotations

import itertools
import math
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

from adam_amd import synth
from adam_amd.records import (F_DUPLICATE, F_HAS_CIGAR, F_HAS_MD, F_HAS_QUAL, F_HAS_REFNAME, F_HAS_RG, F_HAS_SEQ,
                              F_HAS_START, F_MAPPED, F_PRIMARY, RecordBatch)

SEQ_LIMIT = 0.0625          # kFoldSeqLimit: below, the fold adds one by one
TILE_SLOTS, MAX_TILE_READS = 4096, 64   # bqsr_internal.h kTileSlots, kMaxTileReads
POW10 = [math.pow(10.0, -q / 10.0) for q in range(128)]   # phredToErrorProbabilityCache, as oracle/bqsr_oracle.cpp
_POW10 = np.asarray(POW10)


def binade(x: float) -> int:
    """e with 2^e <= x < 2^(e+1) (x > 0)"""
    return math.frexp(x)[1] - 1


def _tie_binade(t: float) -> int:
    m, ex = math.frexp(t)              # t = m * 2^ex, 0.5 <= m < 1
    M = int(m * (1 << 53))             # exact: m has 53 significant bits
    et = ex - 1
    assert M * 2.0 ** (et - 52) == t
    tz = (M & -M).bit_length() - 1
    return et + 1 + tz


TIE_BINADE = [_tie_binade(t) for t in POW10]
_TIE_BINADE = np.asarray(TIE_BINADE)
# per binade -4..4 the largest qual tying there (the smallest tying increment)
TIE_QUAL = {e: max(q for q in range(128) if TIE_BINADE[q] == e) for e in range(-4, 5)}


class FoldRef(NamedTuple):
    em: float                       # the strictly sequential double sum
    n: int                          # folded bases
    ties: List[Tuple[int, int]]     # (index, binade of S before it) of additions with t / u a half-integer, S >= 1/16
    crossings: List[int]            # indices of additions after which S is in another binade, S >= 1/16 before
    seq_end: Optional[int]          # additions made when S first is >= 1/16 (None: never)
    big: List[int]                  # indices of additions of >= 2^52 units (t >= 2^e), S >= 1/16
    partial: np.ndarray             # S after every addition


def ref_fold(quals) -> FoldRef:
    """quals: the folded bases' phred values (0..127) in fold order."""
    q = np.asarray(quals, dtype=np.int64)
    n = int(q.size)
    t = _POW10[q]
    after = np.empty(n, dtype=np.float64)
    s = 0.0
    for a in range(0, n, 1 << 20):      # one addition at a time, in order
        part = list(itertools.accumulate(t[a:a + (1 << 20)].tolist(), initial=s))
        after[a:a + len(part) - 1] = part[1:]
        s = part[-1]
    before = np.concatenate([[0.0], after[:-1]]) if n else after
    on = before >= SEQ_LIMIT
    eb = np.frexp(np.where(on, before, 1.0))[1] - 1
    ea = np.frexp(np.where(on, after, 1.0))[1] - 1
    tie = np.nonzero(on & (_TIE_BINADE[q] == eb))[0]
    reach = np.nonzero(after >= SEQ_LIMIT)[0]
    return FoldRef(em=s, n=n, ties=[(int(i), int(eb[i])) for i in tie],
                   crossings=[int(i) for i in np.nonzero(on & (ea != eb))[0]],
                   seq_end=int(reach[0]) + 1 if reach.size else None,
                   big=[int(i) for i in np.nonzero(on & (t >= np.ldexp(1.0, eb)))[0]], partial=after)


def usable(batch: RecordBatch) -> np.ndarray:
    f = batch.flags
    return ((f & F_MAPPED) != 0) & ((f & F_PRIMARY) != 0) & ((f & F_DUPLICATE) == 0) & ((f & F_HAS_MD) != 0)


def folded_quals(batch: RecordBatch) -> np.ndarray:
    """The partition's folded bases in fold order: every base of every usable
    read between its low-quality ends (phred <= 2 as a Java byte trimmed from
    both ends, ReadCovariates.scala:31-39)."""
    ph = (batch.qual.astype(np.int16) - 33).astype(np.uint8).astype(np.int8)
    off = batch.qual_offset.astype(np.int64)
    use = usable(batch)
    full = off[1:] > off[:-1]
    if full.all() and (ph[off[:-1]] > 2).all() and (ph[off[1:] - 1] > 2).all():   # nothing to trim
        return ph[np.repeat(use, off[1:] - off[:-1])].astype(np.int64)
    out = []
    for r in np.nonzero(use)[0]:
        p = ph[off[r]:off[r + 1]]
        if p.size and p[0] > 2 and p[-1] > 2:
            out.append(p)
            continue
        keep = np.nonzero(p > 2)[0]
        if keep.size:
            out.append(p[keep[0]:keep[-1] + 1])
    return np.concatenate(out).astype(np.int64) if out else np.zeros(0, np.int64)


def folded_counts(batch: RecordBatch) -> np.ndarray:
    """folded bases of every read (the builders keep the reads' ends above phred 2: a usable read folds all)"""
    return np.where(usable(batch), np.diff(batch.qual_offset.astype(np.int64)), 0)


def reads_per_tile(batch: RecordBatch) -> int:
    """finish_batch's tile size: reads of the longest 16-aligned slot span that fit TILE_SLOTS, at most 64"""
    lq = np.diff(batch.qual_offset.astype(np.int64))
    ls = np.diff(batch.seq_offset.astype(np.int64))
    span = int((np.maximum(lq, ls).max() + 15) // 16 * 16) if batch.n_reads else 1
    return max(1, min(MAX_TILE_READS, TILE_SLOTS // max(1, span)))


def block_of_tile(n_tiles: int, nb: int) -> np.ndarray:
    """fold block of every tile: block b holds tiles [n_tiles * b // nb, n_tiles * (b + 1) // nb)"""
    lo = np.arange(nb + 1, dtype=np.int64) * n_tiles // nb
    return np.repeat(np.arange(nb), np.diff(lo))


def tile_of_index(batch: RecordBatch, idx) -> np.ndarray:
    """tile of the idx-th folded base(s)"""
    ends = np.cumsum(folded_counts(batch))
    return np.searchsorted(ends, np.asarray(idx), side="right") // reads_per_tile(batch)


def _all_usable(n_reads, seed, length=100) -> RecordBatch:
    return synth.generate(n_reads, (length,), 1, seed, p_unmapped=0.0, p_duplicate=0.0, p_secondary=0.0,
                          p_q2tail=0.0)


def _set_phred(b: RecordBatch, ph: np.ndarray) -> RecordBatch:
    b.qual = (ph.astype(np.int64) + 33).astype(np.uint8)
    return b


# ---- slow_ties -----------------------------------------------------------------

def slow_ties(n_reads: int = 20000, seed: int = 101) -> RecordBatch:
    """Quals 80..93 (S hardly moves) except one base of q12 in read 0, which
    brings S just over 1/16, and one tying qual per 64 reads: the largest qual
    that ties in the binade S is in then (TIE_QUAL), until S >= 32, where none
    does.  S climbs from 1/16 to 32 through ties alone."""
    b = _all_usable(n_reads, seed)
    rng = np.random.default_rng(seed)
    off = b.qual_offset.astype(np.int64)
    ph = rng.integers(80, 94, int(off[-1]))
    ph[off[0] + 1] = 12
    t = _POW10
    s, done = 0.0, 0
    for k in range(n_reads // 64):
        r = 64 * k + 1 + (7 * k) % 63
        i = int(off[r]) + 1 + (13 * k) % (int(off[r + 1] - off[r]) - 2)   # never a read's first or last base
        for x in t[ph[done:i]].tolist():
            s += x
        e = binade(s)
        if s >= SEQ_LIMIT and e in TIE_QUAL:
            ph[i] = TIE_QUAL[e]
        s += t[ph[i]]
        done = i + 1
    return _set_phred(b, ph)


def slow_ties_prefixes(b: RecordBatch, ref: FoldRef) -> List[int]:
    """Read counts k such that b.slice(0, k) ends right behind the read of the
    last tie of each binade -4..4: a mis-rounded tie is one ulp of its binade,
    which a partition ending there cannot absorb in coarser roundings."""
    ends = np.cumsum(folded_counts(b))
    last = {}
    for i, e in ref.ties:
        last[e] = i
    return [int(np.searchsorted(ends, last[e], side="right")) + 1 for e in sorted(last)]


# ---- low_quals_start -------------------------------------------------------------

def low_quals_start(n_reads: int = 4000, seed: int = 102) -> RecordBatch:
    """Interior quals uniform in 0..13 (every one ties in some binade >= -4, or
    is q0): S runs through 20 binades with ties in the lower ones.  Read 0
    opens q12, q0: an addition of 1.0 at S = 0.063, 2^56 units of its binade."""
    b = _all_usable(n_reads, seed)
    rng = np.random.default_rng(seed)
    off = b.qual_offset.astype(np.int64)
    ph = rng.integers(0, 14, int(off[-1]))
    ph[off[:-1]] = 30
    ph[off[1:] - 1] = 30
    ph[off[0] + 1], ph[off[0] + 2] = 12, 0
    return _set_phred(b, ph)


# ---- sequential_regime / late_crossing / sequential_long ---------------------------

def sequential_regime(n_reads: int = 3000, seed: int = 103) -> RecordBatch:
    """All quals 100..127: S < 1/16 to the end, every addition made one at a time."""
    b = _all_usable(n_reads, seed)
    rng = np.random.default_rng(seed)
    return _set_phred(b, rng.integers(100, 128, int(b.qual_offset[-1])))


def late_crossing(nb: int = 256, seed: int = 104) -> RecordBatch:
    """sequential_regime with q60 in the second half: S reaches 1/16 some
    62 500 bases into it.  Four tiles a block, so that the tile where it does
    can lie between two others of its block."""
    n_reads = 4 * (TILE_SLOTS // 112) * nb
    b = sequential_regime(n_reads, seed)
    ph = b.qual.astype(np.int64) - 33
    ph[int(b.qual_offset[n_reads // 2]):] = 60
    return _set_phred(b, ph)


def sequential_long(seed: int = 105) -> RecordBatch:
    """172 000 reads of quals 100..127: 17.2M folded bases below 1/16, more
    than the event stream's largest capacity (16 MiB), so that the last
    blocks' event segments find no room in it."""
    return sequential_regime(172_000, seed)


# ---- segment_overflow --------------------------------------------------------------

def _long_then_short(n_small: int, seed: int, tie_reads_of) -> RecordBatch:
    """One all-match read of 4096 bases (a tile holds one read then) whose 17
    bases of q0 bring S to 17, then n_small reads of 16 bases of quals 90..100;
    the reads tie_reads_of(n_reads) carry one q7 base, which ties while S is
    in [16, 32)."""
    n = 1 + n_small
    rng = np.random.default_rng(seed)
    lens = np.full(n, 16, np.int64)
    lens[0] = 4096
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    ph = rng.integers(90, 101, int(off[-1]))
    ph[1:18] = 0
    tie_reads = np.asarray(tie_reads_of(n), np.int64)
    ph[off[tie_reads].astype(np.int64) + 1 + tie_reads % 14] = 7      # never a read's first or last base
    seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), int(off[-1]))
    flags = np.full(n, F_MAPPED | F_PRIMARY | F_HAS_RG | F_HAS_MD | F_HAS_QUAL | F_HAS_SEQ | F_HAS_CIGAR |
                    F_HAS_START | F_HAS_REFNAME, np.uint32)
    md = [str(int(l)).encode() for l in lens]
    md_off = np.concatenate([[0], np.cumsum([len(m) for m in md])]).astype(np.uint64)
    return _set_phred(RecordBatch(flags, np.zeros(n, np.int32), np.zeros(n, np.int32), ["chr20"],
                                  1000 + 20 * np.arange(n, dtype=np.int64), off, seq, off.copy(),
                                  np.zeros(int(off[-1]), np.uint8), np.arange(n + 1, dtype=np.uint64),
                                  (lens.astype(np.uint32) << 4), md_off, np.frombuffer(b"".join(md), np.uint8)), ph)


def segment_overflow(nb: int = 256, n_small: Optional[int] = None, seed: int = 106) -> RecordBatch:
    """_long_then_short with n_small (default 140 * nb) short reads.  In every
    eighth block (4, 12, ...) every second read carries the q7 base: the first
    such block alternates tie and tie-free tiles 70 times, more than its
    segment list holds.  From the second one on S >= 32: nothing ties, and the
    blocks between merge."""
    def ties(n):
        blk = block_of_tile(n, nb)                  # reads_per_tile is 1: read r is tile r
        return np.nonzero((blk % 8 == 4) & (np.arange(n) % 2 == 1) & (np.arange(n) > 0))[0]
    return _long_then_short(140 * nb if n_small is None else n_small, seed, ties)


def two_chunks(nb: int = 256, seed: int = 108) -> RecordBatch:
    """_long_then_short with 1100 tiles a block, more than the 1024 that
    bqsr_fold_segs takes at a time; block 4 holds two ties, at its tiles 10 and
    1050: its segments are cut at the chunk border as well."""
    def ties(n):
        first = int(np.nonzero(block_of_tile(n, nb) == 4)[0][0])
        return [first + 10, first + 1050]
    return _long_then_short(1100 * nb, seed, ties)


# ---- empty_blocks ------------------------------------------------------------------

def empty_blocks(n_reads: int = 30000, lo: int = 8000, hi: int = 16000, seed: int = 107) -> RecordBatch:
    """synth.generate's quals; reads lo..hi are unusable (unmapped, duplicate
    or without MD in turn): the blocks inside that range fold nothing."""
    b = _all_usable(n_reads, seed)
    f = b.flags.copy()
    r = np.arange(lo, hi)
    f[r[r % 3 == 0]] &= ~np.uint32(F_MAPPED)
    f[r[r % 3 == 1]] |= np.uint32(F_DUPLICATE)
    f[r[r % 3 == 2]] &= ~np.uint32(F_HAS_MD)
    b.flags = f
    return b


def nobase_blocks(batch: RecordBatch, nb: int) -> np.ndarray:
    """per fold block: True where it holds no folded base (blocks without tiles included)"""
    rpt = reads_per_tile(batch)
    n_tiles = (batch.n_reads + rpt - 1) // rpt
    fc = folded_counts(batch)
    per_tile = np.add.reduceat(fc, np.arange(0, batch.n_reads, rpt)) if batch.n_reads else np.zeros(0, np.int64)
    per_block = np.bincount(block_of_tile(n_tiles, nb), weights=per_tile, minlength=nb)
    return per_block == 0


def longest_true_run_inside(mask: np.ndarray) -> int:
    """longest run of True with a False somewhere before and somewhere after"""
    live = np.nonzero(~mask)[0]
    if live.size < 2:
        return 0
    best = cur = 0
    for v in mask[live[0]:live[-1] + 1]:
        cur = cur + 1 if v else 0
        best = max(best, cur)
    return best


# ---- the cases by name ---------------------------------------------------------------

def small_variants(nb: int = 256) -> List[RecordBatch]:
    """segment_overflow with fewer reads than blocks (blocks without a tile),
    an empty partition, and one read more than blocks"""
    few = segment_overflow(nb, nb // 2 - 1)
    return [few, few.slice(0, 0), segment_overflow(nb, nb)]


_BUILDERS = {
    "slow_ties": lambda nb: slow_ties(),
    "low_quals_start": lambda nb: low_quals_start(),
    "sequential_regime": lambda nb: sequential_regime(),
    "late_crossing": late_crossing,
    "segment_overflow": segment_overflow,
    "two_chunks": two_chunks,
    "empty_blocks": lambda nb: empty_blocks(),
}
CASES = tuple(_BUILDERS)
_cache = {}


def case(name: str, nb: int = 256) -> Tuple[RecordBatch, FoldRef]:
    """the case's batch and its reference fold, built once a session"""
    if (name, nb) not in _cache:
        b = _BUILDERS[name](nb)
        _cache[(name, nb)] = (b, ref_fold(folded_quals(b)))
    return _cache[(name, nb)]
