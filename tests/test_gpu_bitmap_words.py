"""The slot bitmap's private words (bqsr_internal.h, PrepParams): in the
16-aligned slot layout a u32 word per 16-slot chunk belongs to one read, prep
writes the words of the reads that have bits and nothing else, and nothing is
cleared -- not per job, not when the batch is allocated.  So every case here
leaves stale or never-written words next to the ones a job loads, and checks
the job against the CPU oracle bit for bit: table words, expectedMismatch
bits, every output char."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

pytestmark = pytest.mark.gpu


def _md(length, mism):
    """MD of a read of `length` reference bases mismatching at the sorted offsets `mism`."""
    out, prev = [], -1
    for p in mism:
        out.append("%dA" % (p - prev - 1))
        prev = p
    out.append("%d" % (length - prev - 1))
    return "".join(out)


def _read(rng, length, mism=(), cigar=None, md=None, **kw):
    """A crafted read (tests/test_gpu_parity.rec) of `length` bases, quals 30..40."""
    from test_gpu_parity import rec
    seq = "".join(rng.choice(list("ACGT"), size=length))
    qual = "".join(chr(33 + int(q)) for q in rng.integers(30, 41, size=length))
    kw.setdefault("start", 10000 + int(rng.integers(0, 3000)))
    return rec(sequence=seq, qual=qual, cigar=cigar or "%dM" % length,
               mismatching_positions=_md(length, mism) if md is None else md, **kw)


# contig "1", where the crafted reads lie: a site every 7 bases, so every read of 7 bases or more has one
CRAFTED_SITES = {"1": list(range(9990, 13400, 7))}


def _resident_jobs(b, sites, plan):
    """One ResidentJob on one batch, a job per entry of `plan` (with known
    sites or without), each against the oracle."""
    import oracle as O
    from adam_amd import bqsr
    from adam_amd.job import ResidentJob
    snp = bqsr.SnpTable(sites)
    dims = bqsr.dims_of([b])
    od = O.Dims(dims.n_rg, dims.max_len)
    want = {True: O.bqsr(b, O.Sites(sites), od, n_parts=1, nthreads=8, fold1=True),
            False: O.bqsr(b, None, od, n_parts=1, nthreads=8, fold1=True)}
    assert not np.array_equal(want[True][0], want[False][0])  # the sites mask bases
    job = ResidentJob(b, dims, snp, 0)
    sites_h = job.sites_h
    try:
        for i, with_sites in enumerate(plan):
            job.sites_h = sites_h if with_sites else None
            job.step()
            words, em, q, st, ln, exc = job.results()
            ow, oem, out, out_len = want[with_sites]
            assert np.array_equal(words, ow), (i, with_sites)
            assert np.float64(em).tobytes() == np.float64(oem).tobytes(), (i, with_sites)
            bad, first = O.compare_device_output(b, out, out_len, q, st, ln, exc)
            assert bad == 0, (i, with_sites, first)
    finally:
        job.close()


@pytest.mark.parametrize("lens", [(100,), (150, 250)])
def test_stale_bits_on_a_resident_batch(lens):
    # jobs with known sites, without, with, without on one resident batch.  A
    # site every ~32 bases: under sites nearly every read has bits and writes
    # its words; without, about one read in seven does, and the others' words
    # still hold the sites job's bits -- loading one of them would mask bases.
    # 100 bp: the store form (every usable read stores its words) alternates
    # with the register form (only reads with bits do); 150 / 250 bp: the
    # register form (150) and the zero-then-OR form (250) under both.
    from adam_amd import bqsr, synth
    with bqsr.Context.get(0).tuned(order="read"):
        b = synth.generate(12000, lens, 1, seed=301)
        _resident_jobs(b, synth.known_sites(2_000_000, seed=302), (True, False, True, False))


def test_span_parity_and_size():
    # read order; spans of 1 to 16 chunks, odd and even, so reads start on
    # both halves of what was a shared 32-slot word; reads without QUAL and
    # SEQ (span 0, no word at all) in between; the last read ends exactly at
    # n_slots, so the lean observe's 8-word loads run into the column's padding
    from _parity import check
    from adam_amd import bqsr
    from adam_amd.records import RecordBatch
    from test_gpu_parity import rec
    rng = np.random.default_rng(311)
    lens = (1, 16, 17, 96, 100, 128, 129, 160, 250)
    recs = []
    for i in range(4200):
        n = lens[i % len(lens)]
        k = int(rng.integers(0, 4))  # 0: no bit without sites
        mism = sorted(set(int(x) for x in rng.integers(0, n, size=k)))
        recs.append(_read(rng, n, mism, read_negative_strand=bool(i & 2), read_paired=True, second_of_pair=bool(i & 4)))
        if i % 5 == 0:
            recs.append(rec(sequence=None, qual=None, read_mapped=False))
    recs.append(_read(rng, 160, (0, 159)))  # ends at n_slots
    b = RecordBatch.from_records(recs)
    with bqsr.Context.get(0).tuned(order="read"):
        check([b], CRAFTED_SITES)
        check([b])


def _writers():
    """Reads for every code path that writes bitmap words."""
    from test_gpu_parity import EDGE
    rng = np.random.default_rng(321)
    recs = list(EDGE)
    for n in (100, 150, 250):
        m = n - 10
        recs += [
            _read(rng, n, cigar="5S%dM5S" % m, md=_md(m, (0, 7, m - 1))),                         # soft clips
            _read(rng, n, cigar="3H5S%dM5S2H" % m, md=_md(m, ())),                                # hard and soft clips
            _read(rng, n, cigar="40M10I%dM" % (n - 50), md=_md(n - 10, (39, 40))),                # insertion
            _read(rng, n, cigar="40M3D%dM" % (n - 40), md="40^ACG%d" % (n - 40)),                 # deletion
            _read(rng, n, cigar="2S38M2I%dM4S" % (n - 46), md=_md(n - 8, (1, 37, 38, n - 9))),    # clips and an insertion
            _read(rng, n, cigar="20M1I20M1D%dM" % (n - 41), md="40^T%d" % (n - 41)),              # two indels: the per-read path
            _read(rng, n, mism=range(3, 3 + 2 * 9, 2)),                                           # 9 mismatches, MD over 16 bytes
            _read(rng, n, mism=range(0, n, 2)),                                                   # MD far over 32 bytes
            _read(rng, n, mism=(5, 50, 60, 70, 80, 90), read_negative_strand=True),               # MD of 17..32 bytes
            _read(rng, n, md="%d" % (n // 2)),                                                    # MD shorter than the span
            _read(rng, n, mism=(n - 1,), read_negative_strand=True, read_paired=True, second_of_pair=True),
            _read(rng, n, mism=(0,), read_paired=True, second_of_pair=True),
            _read(rng, n),                                                                        # no bit without sites
        ]
        # Q2 tails, every trimmed base a mismatch: the listed reads (the long form, then the per-read path)
        for tail, extra in ((6, ()), (12, (4,)), (20, (1, 3, 5, 7, 9, 11, 13, 15, 17))):
            r = _read(rng, n, mism=tuple(extra) + tuple(range(n - tail, n)))
            r.qual = r.qual[:n - tail] + "#" * tail
            recs.append(r)
    return recs


@pytest.mark.parametrize("with_sites", [True, False])
def test_every_writer(with_sites):
    # three copies, so the reads of each kind sit at several spans' offsets and in more than one wavefront
    from _parity import check
    from adam_amd import bqsr
    from adam_amd.records import RecordBatch
    recs = _writers()
    b = RecordBatch.from_records(recs + recs[::-1] + recs)
    sites = dict(CRAFTED_SITES)
    sites["1"] = sorted(set(sites["1"] + [10002, 10005, 40, 44, 10013]))
    with bqsr.Context.get(0).tuned(order="read"):
        check([b], sites if with_sites else None)
    check([b.slice(0, len(recs)), b.slice(len(recs), b.n_reads)], sites if with_sites else None)


def test_bucketed_order():
    # bucketed by read group: bqsr_observe_chunks loads one u32 word per chunk
    # at the read's own slot, with sites (most reads have bits) and without
    from adam_amd import bqsr, synth
    with bqsr.Context.get(0).tuned(order="group"):
        b = synth.generate(8000, (150, 250), 8, seed=331)
        _resident_jobs(b, synth.known_sites(2_000_000, seed=332), (True, False, True))


def test_streamed_shard():
    # two partitions of one shape through the streamed path, twice: the first
    # with clips, an insertion and mismatches on every read, the second all
    # matches -- none of its reads writes a word, and whatever its bitmap's
    # allocation holds (the first partition's pattern, if the allocator hands
    # the same memory out again) is never loaded
    import torch
    from _parity import run_oracle
    from adam_amd import _capi, bqsr
    from adam_amd.records import RecordBatch
    from adam_amd.stream import StreamedShard
    from test_gpu_stream import _slots
    rng = np.random.default_rng(341)
    n = 3000
    first = RecordBatch.from_records(
        [_read(rng, 100, cigar="4S40M2I50M4S", md=_md(90, (0, 11, 39, 40, 89))) for _ in range(n)])
    second = RecordBatch.from_records([_read(rng, 100) for _ in range(n)])
    parts = [first, second]
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    d = bqsr.dims_of(parts)
    ctx = bqsr.Context.get(0)
    L = _capi.lib()
    words_t = torch.zeros(int(L.bqsr_table_words(d)), dtype=torch.int64, device=dev)
    th = ctypes.c_void_p()
    _capi.check(L.bqsr_table_create(ctx.handle, d, ctypes.c_void_p(words_t.data_ptr()), ctypes.byref(th)))
    o = run_oracle(parts, None)
    for order in ((0, 1), (1, 0)):  # a shard freed, then one with the partitions the other way round
        ps = [parts[i] for i in order]
        sh = StreamedShard(ctx, ps, d, None, 0)
        try:
            for _ in range(2):
                em_t = sh.run(th)
                assert sh.finish() == 0
            assert np.array_equal(words_t.cpu().numpy(), o.words)
            assert sh.em.cpu().numpy()[:2].tolist() == [o.parts_em[i] for i in order]
            for k, i in enumerate(order):
                ref_out, ref_len = o.outs[i]
                slots = _slots(ps[k])
                for r in range(n):
                    a = int(ps[k].qual_offset[r])
                    assert np.array_equal(sh.qual_chars(k, int(slots[r]), r), ref_out[a:a + int(ref_len[r])]), (i, r)
        finally:
            sh.close()
    L.bqsr_table_destroy(th)
