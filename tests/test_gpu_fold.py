"""The expectedMismatch fold (adam_amd/csrc/bqsr_fold.hip) on the inputs of
tests/_fold_cases.py: ties at every binade they exist in, a sequential regime
longer than the chain's LDS prefetch, 1/16 reached in the middle of a block,
a block with more segments than its list holds, blocks that fold nothing,
fewer tiles than blocks, blocks of more tiles than bqsr_fold_segs takes at a
time, and more event bytes than the stream holds.

Every run is compared bit for bit with the CPU oracle (table words and each
partition's expectedMismatch) and with the one-addition-at-a-time reference
(ref_fold); then bqsr_batch_fold_stats tells whether the job took the path
the case exists for.  tests/test_fold_cases.py checks, without a GPU, that
the inputs demand those paths.

The stream's capacity is max(1 MiB, min(16 MiB, slots)).  Event bytes never
exceed the folded bases, which are at most the slots, and a block's <= 63
event segments add < 63 * 64 B of padding each block: 256 * 63 * 64 B < 1 MiB.
So the capacity is only exceeded by event bytes beyond 16 MiB:
test_stream_capacity folds 17.2M bases that never reach 1/16.

The chain prefetches 384 segments.  A block in the sequential regime is one
event segment, so sequential_regime's 84 tiles cannot pass that limit; the
segments beyond it are slow_ties' (a tie in every second tile of more than 200
candidate blocks).
"""
import ctypes
import struct

import numpy as np
import pytest

import _fold_cases as F
from _parity import assert_same, run_gpu, run_oracle
from adam_amd import _capi, bqsr, synth

pytestmark = pytest.mark.gpu


def bits(x):
    return struct.pack("<d", x)


@pytest.fixture(scope="module")
def nb():
    """fold blocks: one per CU (bqsr_capi.cpp finish_batch)"""
    import torch
    return min(torch.cuda.get_device_properties(0).multi_processor_count, 1024)


@pytest.fixture
def read_order(request):
    """BQSR_TUNE_ORDER: 'read' = the observe kernel (bqsr_observe_chunks or
    bqsr_observe_lean) leaves the blocks' qual histograms, 'group' = bucketed
    passes, the histograms from bqsr_fold_hist"""
    with bqsr.Context.get(0).tuned(order=request.param):
        yield request.param


def observe_jobs(batch, sites=None, jobs=1):
    """`jobs` observe jobs on one device batch, as the staged path runs them:
    per job the table words, expectedMismatch and the fold's stats."""
    import torch
    ctx = bqsr.Context.get(0)
    L = _capi.lib()
    snp = bqsr.SnpTable(sites) if sites else None
    d = bqsr.dims_of([batch])
    dev = torch.device("cuda", 0)
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    s, keep = batch.c_struct(batch.contig_ids_for(snp.contigs if snp else None))
    bh, th = ctypes.c_void_p(), ctypes.c_void_p()
    _capi.check(L.bqsr_batch_create(ctx.handle, ctypes.byref(s), sp, ctypes.byref(bh)))
    out = []
    try:
        st = _capi.FoldStats()
        assert L.bqsr_batch_fold_stats(bh, ctypes.byref(st), sp) == _capi.INVALID_ARG   # no fold yet
        words_t = torch.zeros(int(L.bqsr_table_words(d)), dtype=torch.int64, device=dev)
        _capi.check(L.bqsr_table_create(ctx.handle, d, ctypes.c_void_p(words_t.data_ptr()), ctypes.byref(th)))
        for _ in range(jobs):
            _capi.check(L.bqsr_table_zero_async(th, sp))
            _capi.check(L.bqsr_observe_async(ctx.handle, bh, snp.handle(ctx) if snp else None, th, sp))
            em = ctypes.c_double()
            _capi.check(L.bqsr_observe_result(bh, ctypes.byref(em), sp))
            st = _capi.FoldStats()
            _capi.check(L.bqsr_batch_fold_stats(bh, ctypes.byref(st), sp))
            print({f: getattr(st, f) for f, _ in st._fields_})
            out.append((words_t.cpu().numpy(), em.value, st))
    finally:
        if th:
            L.bqsr_table_destroy(th)
        L.bqsr_batch_destroy(bh)
    return out


def event_blocks(batch, ref, nb):
    """blocks that hold an addition below 1/16, a tie or a crossing: candidates whatever the bounds"""
    rpt = F.reads_per_tile(batch)
    blk = F.block_of_tile((batch.n_reads + rpt - 1) // rpt, nb)
    idx = [i for i, _ in ref.ties] + ref.crossings
    tiles = set(F.tile_of_index(batch, idx).tolist()) if idx else set()
    last_seq = (ref.seq_end if ref.seq_end is not None else ref.n) - 1
    tiles |= set(range(int(F.tile_of_index(batch, last_seq)) + 1))
    return {int(blk[t]) for t in tiles} - set(np.nonzero(F.nobase_blocks(batch, nb))[0].tolist())


def check_stats_consistent(st, batch, nb, ref=None):
    rpt = F.reads_per_tile(batch)
    if ref is not None:
        assert st.cand_blocks >= len(event_blocks(batch, ref, nb))
    assert (st.n_blocks, st.reads_per_tile, st.n_tiles) == (nb, rpt, (batch.n_reads + rpt - 1) // rpt)
    assert st.segs_total == st.segs_run + st.segs_event + st.segs_global
    assert st.segs_refused <= st.segs_global and st.capped_blocks <= st.cand_blocks <= nb
    assert st.nobase_blocks == int(F.nobase_blocks(batch, nb).sum())
    assert st.tileless_blocks == sum(st.n_tiles * b // nb == st.n_tiles * (b + 1) // nb for b in range(nb))
    assert (st.lds_stream, st.lds_segs) == (80 * 1024, 384)
    assert st.stream_cap == max(1 << 20, min(16 << 20, int(bqsr_slots(batch))))


def bqsr_slots(batch):
    span = np.maximum(np.diff(batch.qual_offset.astype(np.int64)), np.diff(batch.seq_offset.astype(np.int64)))
    return ((span + 15) // 16 * 16).sum()


def expect_path(name, st, batch, nb):
    """the path the case exists for"""
    tiled = nb - st.tileless_blocks
    if name == "slow_ties":
        assert st.segs_event > 0 and st.segs_run > 0      # tie tiles and tie-free tiles inside candidate blocks
        assert st.longest_run > 1                         # the blocks past S = 32 merge
        if nb == 256:
            assert st.segs_total > st.lds_segs            # segments the chain reads from global memory
    elif name == "low_quals_start":
        assert st.segs_event >= 2                         # (its q0 and ties all lie in the first tile)
    elif name == "sequential_regime":
        assert st.stream_used > st.lds_stream             # streams folded through the chain's scratch buffer
        assert st.cand_blocks == tiled and st.segs_event == st.segs_total == tiled   # every tile an event
    elif name == "late_crossing":
        assert st.stream_used > st.lds_stream
        assert tiled // 2 <= st.cand_blocks < tiled and st.segs_run > 0 and st.longest_run > 1
    elif name == "segment_overflow":
        assert st.capped_blocks >= 1 and st.segs_global >= 1 and st.segs_refused == 0
        assert st.longest_run >= 7                        # the seven blocks between two tie blocks
    elif name == "two_chunks":
        # block 0: the long read's tile, then tie-free tiles cut at tile 1024; block 4: cut by its two ties
        # and at tile 1024 -- one segment more each than the keys alone would give
        assert (st.cand_blocks, st.segs_event, st.segs_run, st.segs_total) == (2, 3, 6, 9)
        assert st.n_tiles > 1024 * nb and st.longest_run == nb - 5
    elif name == "empty_blocks":
        assert st.nobase_between >= 32 * nb // 256
    assert st.stream_used <= st.stream_cap and st.segs_refused == 0


@pytest.mark.parametrize("read_order", ["read", "group"], indirect=True)
@pytest.mark.parametrize("name", F.CASES)
def test_fold_case(name, read_order, nb):
    b, ref = F.case(name, nb)
    o = run_oracle([b], stage="observe")
    g = run_gpu([b], stage="observe")
    print(name, read_order, "gpu", g.parts_em, "oracle", o.parts_em, "ref", ref.em)
    assert_same([b], g, o)
    assert bits(g.parts_em[0]) == bits(o.parts_em[0]) == bits(ref.em)
    (words, em, st), = observe_jobs(b)
    assert np.array_equal(words, o.words) and bits(em) == bits(ref.em)
    check_stats_consistent(st, b, nb, ref)
    expect_path(name, st, b, nb)


@pytest.mark.parametrize("read_order", ["read", "group"], indirect=True)
def test_slow_ties_prefixes(read_order, nb):
    """partitions ending right behind the last tie of each binade -4..4: one
    mis-rounded tie is one ulp of a result in that binade or the next"""
    b, ref = F.case("slow_ties", nb)
    ks = F.slow_ties_prefixes(b, ref)
    ends = np.cumsum(F.folded_counts(b))
    parts = [b.slice(0, k) for k in ks]
    o = run_oracle(parts, stage="observe")
    g = run_gpu(parts, stage="observe")
    want = [float(ref.partial[ends[k - 1] - 1]) for k in ks]
    print("gpu", g.parts_em, "oracle", o.parts_em, "ref", want)
    assert_same(parts, g, o)
    assert [bits(x) for x in g.parts_em] == [bits(x) for x in o.parts_em] == [bits(x) for x in want]


@pytest.mark.parametrize("read_order", ["read"], indirect=True)
def test_slow_ties_known_sites(read_order, nb):
    """known sites mask bases out of the table, never out of the fold"""
    b, ref = F.case("slow_ties", nb)
    sites = synth.known_sites(2_000_000, seed=5)
    o = run_oracle([b], sites, stage="observe")
    g = run_gpu([b], sites, stage="observe")
    assert_same([b], g, o)
    assert bits(g.parts_em[0]) == bits(ref.em)
    assert not np.array_equal(o.words, run_oracle([b], stage="observe").words)   # the sites do mask something
    (words, em, st), = observe_jobs(b, sites)
    assert np.array_equal(words, o.words) and bits(em) == bits(ref.em)
    expect_path("slow_ties", st, b, nb)


@pytest.mark.parametrize("read_order", ["read", "group"], indirect=True)
def test_small_variants(read_order, nb):
    """fewer reads (tiles) than blocks, an empty partition, one read more than blocks"""
    parts = F.small_variants(nb)
    o = run_oracle(parts, stage="observe")
    g = run_gpu(parts, stage="observe")
    assert_same(parts, g, o)
    for p, em in zip(parts, g.parts_em):
        assert bits(em) == bits(F.ref_fold(F.folded_quals(p)).em)
    few, _, more = parts
    (words, em, st), = observe_jobs(few)
    check_stats_consistent(st, few, nb)
    assert bits(em) == bits(g.parts_em[0]) and st.tileless_blocks == nb - few.n_reads > 0
    assert st.nobase_blocks == st.tileless_blocks and st.cand_blocks >= 1
    (words, em, st), = observe_jobs(more)
    check_stats_consistent(st, more, nb)
    assert bits(em) == bits(g.parts_em[2]) and st.tileless_blocks == 0 and st.n_tiles == nb + 1


@pytest.mark.parametrize("name", ["slow_ties", "sequential_regime"])
def test_second_job_on_the_batch(name, nb):
    """two jobs on one device batch (the staged path's steady state): the
    fold's counters, segment lists and streams are rebuilt, not accumulated"""
    b, ref = F.case(name, nb)
    o = run_oracle([b], stage="observe")
    first, second = observe_jobs(b, jobs=2)
    for words, em, st in (first, second):
        assert np.array_equal(words, o.words) and bits(em) == bits(ref.em)
        expect_path(name, st, b, nb)
    assert bytes(first[2]) == bytes(second[2])


@pytest.mark.parametrize("read_order", ["read"], indirect=True)
def test_stream_capacity(read_order, nb):
    """17.2M folded bases below 1/16: the last blocks' event segments find no
    room in the 16 MiB stream and are folded from the read columns"""
    b = F.sequential_long()
    want = F.ref_fold(F.folded_quals(b)).em
    (words, em, st), = observe_jobs(b)
    print("gpu", em, "ref", want)
    o = run_oracle([b], stage="observe")
    assert np.array_equal(words, o.words) and bits(em) == bits(o.em) == bits(want)
    assert st.stream_cap == 16 << 20 and st.stream_used > st.stream_cap
    assert st.segs_refused >= 1 and st.segs_global == st.segs_refused and st.cand_blocks == nb
