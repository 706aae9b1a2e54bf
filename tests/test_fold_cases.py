"""The fold cases of tests/_fold_cases.py, without a GPU: the sequential
reference equals the CPU oracle's expectedMismatch bit for bit on every case
(which checks builder, folded-base extraction and reference against the C++
restatement), and every case demands the path it exists for.  The device runs
of the same cases are tests/test_gpu_fold.py.

nb = 256 fold blocks (one per CU of an MI355X) here; the GPU tests take the
block count from the device.
"""
import collections
import ctypes
import os

import numpy as np
import pytest

import oracle as O
import _fold_cases as F
from adam_amd import _capi

NB = 256
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "adam_bqsr.h")


def _oracle_em(b):
    return O.observe(b, None, O.Dims(1, b.max_len()))[1]


# ---- the tie table -------------------------------------------------------------------

def test_tie_binades_from_the_bits():
    # the quals that can tie at S >= 1/16, and where (derived in _fold_cases from the doubles' bits)
    want = {1: 2, 2: 3, 3: 1, 4: 0, 5: -1, 6: 1, 7: 4, 8: -2, 9: 2, 10: -2, 11: -1, 12: -2, 13: -4, 14: -3, 15: -3,
            16: -4, 17: -4, 18: -3, 21: -2, 22: -1, 24: -4}
    assert {q: e for q, e in enumerate(F.TIE_BINADE) if q > 0 and e >= -4} == want
    assert max(F.TIE_BINADE[1:]) == 4          # no tie once S >= 32 ...
    assert F.TIE_BINADE[0] == 53               # ... but q0's, at S >= 2^53
    assert F.TIE_QUAL == {-4: 24, -3: 18, -2: 21, -1: 22, 0: 4, 1: 6, 2: 9, 3: 2, 4: 7}
    # the definition, in exact rational arithmetic: t / 2^(e-52) is a half-integer at that binade only
    from fractions import Fraction
    for q, t in enumerate(F.POW10):
        for e in range(-8, 8):
            x = Fraction(t) / Fraction(2) ** (e - 52)
            assert ((2 * x).denominator == 1 and x.denominator == 2) == (F.TIE_BINADE[q] == e), (q, e)
    assert [O.pow10cache(q) for q in range(128)] == F.POW10


def test_ref_fold_on_a_hand_case():
    # 0.0631 (q12) -> +1.0 (q0: 2^56 units of binade -4, a crossing) -> +q4 at S in [1, 2): a tie
    r = F.ref_fold([40, 12, 0, 4, 40])
    assert r.em == (((F.POW10[40] + F.POW10[12]) + 1.0) + F.POW10[4]) + F.POW10[40]
    assert (r.seq_end, r.big, r.crossings, r.ties) == (2, [2], [2], [(3, 0)])
    assert F.ref_fold([]).em == 0.0 and F.ref_fold([]).seq_end is None


def test_folded_quals_trims_as_the_oracle():
    # low-quality tails, unusable reads: folded_quals' general path
    from adam_amd import synth
    b = synth.generate(3000, (100,), 2, seed=9, p_q2tail=0.4)
    assert not F.usable(b).all()
    q = F.folded_quals(b)
    assert q.size < int(F.folded_counts(b).sum())          # something was trimmed
    assert F.ref_fold(q).em == O.observe(b, None, O.Dims(2, b.max_len()))[1]


# ---- every case: reference == oracle, all reads usable and untrimmed -------------------

@pytest.mark.parametrize("name", F.CASES)
def test_reference_equals_oracle(name):
    b, ref = F.case(name, NB)
    assert ref.em == _oracle_em(b)
    assert ref.n == int(F.folded_counts(b).sum())          # no trimming: usable reads fold every base
    if name != "empty_blocks":
        assert F.usable(b).all() and ref.n == int(b.qual_offset[-1])


def test_small_variants_reference_equals_oracle():
    few, empty, more = F.small_variants(NB)
    assert few.n_reads < NB and empty.n_reads == 0 and more.n_reads == NB + 1
    for p in (few, more):
        assert F.reads_per_tile(p) == 1
        assert F.ref_fold(F.folded_quals(p)).em == _oracle_em(p)
    assert F.nobase_blocks(few, NB).sum() == NB - few.n_reads    # blocks without a tile


# ---- the conditions each case exists for ----------------------------------------------------

def test_slow_ties_conditions():
    b, ref = F.case("slow_ties", NB)
    per = collections.Counter(e for _, e in ref.ties)
    assert len(ref.ties) >= 200
    assert all(per[e] >= 3 for e in range(-4, 5)), per
    assert len(set(F.tile_of_index(b, [i for i, _ in ref.ties]).tolist())) >= 200
    assert len(ref.crossings) == 9 and ref.seq_end <= 200 and 32.0 <= ref.em < 64.0
    # the prefixes: one ends inside (or one binade above) each tie binade, right behind that binade's last tie
    ks = F.slow_ties_prefixes(b, ref)
    assert len(ks) == 9 and ks == sorted(set(ks)) and ks[-1] < b.n_reads
    ends = np.cumsum(F.folded_counts(b))
    for e, k in zip(range(-4, 5), ks):
        s = float(ref.partial[ends[k - 1] - 1])
        last = [t for t in ref.ties if t[0] < ends[k - 1]][-1]
        assert last[1] == e and F.binade(s) - e in (0, 1), (e, k, s)
        assert s == O.em_fold(b, 0, k)


def test_low_quals_start_conditions():
    b, ref = F.case("low_quals_start", NB)
    assert len([t for t in ref.ties]) >= 8
    assert len(ref.crossings) >= 10
    q = F.folded_quals(b)
    big_q0 = [i for i in ref.big if q[i] == 0 and 0.0625 <= ref.partial[i - 1] < 2.0]
    assert big_q0, "no q0 base added while 1/16 <= S < 2"


def test_sequential_regime_conditions():
    b, ref = F.case("sequential_regime", NB)
    assert ref.seq_end is None and ref.em < F.SEQ_LIMIT and not ref.ties and not ref.crossings
    assert ref.n == 300_000 and ref.n > 80 * 1024          # more folded bytes than the chain prefetches


def test_late_crossing_conditions():
    b, ref = F.case("late_crossing", NB)
    assert ref.seq_end is not None and ref.seq_end > ref.n // 2 + 60_000
    assert ref.seq_end % 64 != 0
    rpt = F.reads_per_tile(b)
    n_tiles = (b.n_reads + rpt - 1) // rpt
    blk = F.block_of_tile(n_tiles, NB)
    tl = int(F.tile_of_index(b, ref.seq_end - 1))
    assert blk[tl - 1] == blk[tl] == blk[tl + 1]           # neither the first nor the last tile of its block


def test_segment_overflow_conditions():
    b, ref = F.case("segment_overflow", NB)
    assert F.reads_per_tile(b) == 1 and b.n_reads == 1 + 140 * NB
    blk = F.block_of_tile(b.n_reads, NB)                   # a tile is a read
    tie_tiles = F.tile_of_index(b, [i for i, _ in ref.ties])
    assert set((blk[tie_tiles] % 8).tolist()) == {4}       # the other seven blocks per eight hold none
    ends = np.cumsum(F.folded_counts(b))
    tiles = np.nonzero(blk == 4)[0]
    s0, s1 = ref.partial[ends[tiles[0] - 1] - 1], ref.partial[ends[tiles[-1]] - 1]
    assert 16.0 <= s0 < s1 < 32.0                          # S stays in [16, 32) over block 4
    has = np.isin(tiles, tie_tiles)
    assert int((has[1:] != has[:-1]).sum()) >= 65          # tie / tie-free alternations inside it
    assert all(e == 4 for _, e in ref.ties)
    # from the second such block on S >= 32: its blocks hold no event but a crossing now and then
    assert ref.partial[ends[np.nonzero(blk == 12)[0][-1]] - 1] >= 32.0


def test_two_chunks_conditions():
    b, ref = F.case("two_chunks", NB)
    assert F.reads_per_tile(b) == 1
    blk = F.block_of_tile(b.n_reads, NB)
    tiles = np.nonzero(blk == 4)[0]
    assert len(tiles) > 1024                               # more tiles than one pass of bqsr_fold_segs takes
    tie_tiles = F.tile_of_index(b, [i for i, _ in ref.ties])
    assert [(int(t - tiles[0]), e) for t, (_, e) in zip(tie_tiles, ref.ties)] == [(10, 4), (1050, 4)]
    assert ref.crossings and max(ref.crossings) < 4096 and 16.0 <= ref.em < 32.0   # S in [16, 32) behind read 0


def test_empty_blocks_conditions():
    b, ref = F.case("empty_blocks", NB)
    assert F.longest_true_run_inside(F.nobase_blocks(b, NB)) >= 32


def test_sequential_long_exceeds_the_stream():
    """stream_cap = max(1 MiB, min(16 MiB, slots)): the 17.2M event bytes of
    a partition that never reaches 1/16 do not fit 16 MiB."""
    b = F.sequential_long()
    ref = F.ref_fold(F.folded_quals(b))
    slots = 112 * b.n_reads
    assert ref.seq_end is None and ref.n > (16 << 20) and slots > (16 << 20)
    assert ref.em == _oracle_em(b)


# ---- the stats call's ABI -------------------------------------------------------------------------

def test_fold_stats_symbol_and_struct():
    assert "bqsr_batch_fold_stats" in _capi.EXPORTS
    assert hasattr(ctypes.CDLL(_capi.LIB_PATH), "bqsr_batch_fold_stats")
    with open(HEADER) as fh:
        text = fh.read()
    body = text[text.index("typedef struct bqsr_fold_stats {"):text.index("} bqsr_fold_stats;")]
    decl = [l.split(";")[0].split() for l in body.splitlines()[1:] if ";" in l]
    assert [d[-1] for d in decl] == [f for f, _ in _capi.FoldStats._fields_]
    ctype = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}
    assert [ctype[d[0]] for d in decl] == [t for _, t in _capi.FoldStats._fields_]
    assert ctypes.sizeof(_capi.FoldStats) == 4 * 8 + 14 * 4
