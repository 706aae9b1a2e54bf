"""MarkDuplicates (§8 f3): the library's bqsr_mark_duplicates (host C++, no
device) against the cases of core/.../rdd/MarkDuplicatesSuite.scala:27-166 and
against the plain-Python restatement in oracle/markdup.py on random read sets."""

import numpy as np
import pytest

import markdup as M  # oracle/markdup.py (tests/conftest.py puts oracle/ on sys.path)
import _markdup_gen as G
from _markdup_gen import mapped, pair


def suite(name):
    """The reads of one MarkDuplicatesSuite case (tests/_markdup_gen.py holds them for every path)."""
    return G.REFERENCE_SUITE[name]()[0]


def run(reads):
    got = G.host_mark(reads)
    want = M.mark_duplicates(reads)
    assert list(got) == want
    return got


def test_single_read():
    assert not run(suite("single_read")).any()


def test_reads_at_different_positions():
    assert not run(suite("reads_at_different_positions")).any()


def test_reads_at_the_same_position():
    d = run(suite("reads_at_the_same_position"))
    assert len(d) == 11
    assert not d[0] and d[1:].all()


def test_reads_at_the_same_position_with_clipping():
    d = run(suite("reads_at_the_same_position_with_clipping"))
    assert len(d) == 11
    assert not d[0] and d[1:].all()


def test_reads_on_reverse_strand():
    d = run(suite("reads_on_reverse_strand"))
    assert len(d) == 8
    assert not d[0] and d[1:].all()


def test_unmapped_reads():
    d = run(suite("unmapped_reads"))
    assert len(d) == 10 and not d.any()


def test_read_pairs():
    d = run(suite("read_pairs"))
    assert len(d) == 22
    assert not d[:2].any() and d[2:].all()


def test_read_pairs_with_fragments():
    d = run(suite("read_pairs_with_fragments"))
    assert len(d) == 12
    assert d[:10].all() and not d[10:].any()


def test_quality_score():
    assert M.score(dict(qual=chr(53) * 100)) == 2000


@pytest.mark.parametrize("seed", range(6))
def test_random_reads_against_restatement(seed):
    rng = np.random.default_rng(seed)
    reads = []
    for k in range(400):
        kind = rng.integers(0, 10)
        name = "q%d" % rng.integers(0, 150)
        lib = [None, "libA", "libB"][rng.integers(0, 3)]
        rg = [None, 0, 1][rng.integers(0, 3)]
        clip = int(rng.integers(0, 3)) * int(rng.integers(0, 6))
        cig = ([(clip, "S")] if clip else []) + [(int(rng.integers(20, 60)), "M")]
        if rng.integers(0, 4) == 0:
            cig += [(int(rng.integers(1, 4)), "D"), (int(rng.integers(5, 20)), "M"), (int(rng.integers(1, 5)), "H")]
        r = dict(name=name, library=lib, rg=rg, mapped=kind != 0, primary=kind != 1, paired=bool(rng.integers(0, 2)),
                 mate_mapped=bool(rng.integers(0, 2)), neg=bool(rng.integers(0, 2)), ref=int(rng.integers(0, 2)),
                 start=int(rng.integers(0, 30)),
                 qual="".join(chr(33 + int(q)) for q in rng.integers(0, 45, size=int(rng.integers(0, 40)))),
                 cigar=cig)
        reads.append(r)
    run(reads)


def test_tied_best_buckets_equivalent():
    """Equally scored best buckets (MarkDuplicates.scala:67-92 sortBy over a
    Spark group, whose order is the shuffle's): any one of them may stay
    unmarked.  The library keeps the first in input order, as the oracle."""
    reads = [mapped(1, 42, phred=30, name="a"), mapped(1, 42, phred=30, name="b"), mapped(1, 42, name="c")]
    d = run(reads)
    assert list(d) == [False, True, True]
    ok, why = M.equivalent_marks(reads, [True, False, True])  # the other tied bucket kept
    assert ok, why
    assert not M.equivalent_marks(reads, [False, False, True])[0]  # both kept
    assert not M.equivalent_marks(reads, [True, True, True])[0]    # none kept
    assert not M.equivalent_marks(reads, [True, False, False])[0]  # the poorer read is no tie
    pairs = pair(0, 10, 0, 210, name="p", phred=30) + pair(0, 10, 0, 210, name="q", phred=30)
    run(pairs)
    assert M.equivalent_marks(pairs, [True, True, False, False])[0]
    assert not M.equivalent_marks(pairs, [True, False, False, True])[0]  # a bucket split
