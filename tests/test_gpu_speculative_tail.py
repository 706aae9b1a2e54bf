"""The speculative job tail (bqsr_job_tail_async): apply starts on
tables finalized from an estimate of expectedMismatch while the exact fold
runs beside it, the exact tables are compared afterwards and apply runs again
on the device if a char could differ.  Whatever it does, a job's results are
those of the serial schedule bit for bit: every case runs BQSR_TUNE_SPEC_TAIL
0 (serial), 1 (speculative) and 2 (speculative, apply always redone) on one
input and compares everything ResidentJob.results() and bqsr_job_result
return -- table words, expectedMismatch bits, the recalibrated chars with
their start and length, the exception list and count, finalize's globals, the
LUT's a2 / s1 / d2, the error raised -- and asserts which schedule ran
(bqsr_job_tail_path).  spec_tail=3 multiplies the estimate by 1.5 on an input
built so that this changes chars: the compare kernel must see it."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

pytestmark = pytest.mark.gpu

SERIAL, SPEC, REDONE = 0, 1, 2


def _snapshot(job):
    """everything a job leaves, in comparable form"""
    from adam_amd import _capi
    L = _capi.lib()
    words, em, q, st, ln, exc = job.results()
    # chars inside each read's [start, start + len): the other slots are scratch
    b = job.batch
    lq = (b.qual_offset[1:] - b.qual_offset[:-1]).astype(np.int64)
    ls = (b.seq_offset[1:] - b.seq_offset[:-1]).astype(np.int64)
    span = (np.maximum(lq, ls) + 15) // 16 * 16
    slot = np.concatenate([[0], np.cumsum(span)])[:-1]
    chars = [q[int(s + a):int(s + a + n)].tobytes() for s, a, n in zip(slot, st, ln)]
    snap = dict(words=words.tobytes(), em=np.float64(em).tobytes(), chars=chars, start=st.tobytes(), len=ln.tobytes(),
                exc=np.sort(exc).tobytes(), n_exc=job.n_exc)
    if job.lut:
        fs = _capi.FinalStats()
        _capi.check(L.bqsr_lut_stats(job.lut, ctypes.byref(fs)))
        snap["final"] = (np.float64(fs.average_reported_error).tobytes(), np.float64(fs.global_error).tobytes(),
                         fs.global_obs, fs.global_mm)
        n_rq, C = job.dims.n_rg * 128, 2 * job.dims.max_len + 1
        a2, s1, d2 = np.zeros(n_rq), np.zeros(n_rq * C), np.zeros(n_rq * 21)
        _capi.check(L.bqsr_lut_tables(job.lut, a2.ctypes.data, s1.ctypes.data, d2.ctypes.data))
        snap.update(a2=a2.tobytes(), s1=s1.tobytes(), d2=d2.tobytes())
    return snap


def _step(job, mode, step=None):
    """one job under spec_tail=mode: (snapshot, error name or None, tail path)"""
    from adam_amd import _capi, bqsr
    err = None
    with bqsr.Context.get(0).tuned(spec_tail=mode):
        try:
            (step or job.step)()
        except _capi.BQSRError as e:
            err = (e.status, e.read)
    return _snapshot(job), err, job.tail_path


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k == "chars":
            bad = [i for i, (x, y) in enumerate(zip(a[k], b[k])) if x != y]
            assert not bad, "reads %s differ" % bad[:10]
        else:
            assert a[k] == b[k], k
    return True


def _three_ways(batch, snp=None, dims=None, step=None, expect_error=False, paths=(SERIAL, SPEC, REDONE)):
    """serial, speculative, speculative with the redo on one batch; returns the serial snapshot"""
    from adam_amd import bqsr
    from adam_amd.job import ResidentJob
    job = ResidentJob(batch, dims or bqsr.dims_of([batch]), snp, 0)
    try:
        bound = (lambda: step(job)) if step else None
        ref, err0, p0 = _step(job, 0, bound)
        assert p0 == SERIAL
        assert (err0 is not None) == expect_error, err0
        for mode in (1, 2):
            got, err, path = _step(job, mode, bound)
            assert path == paths[mode], (mode, path)
            assert err == err0, (mode, err, err0)
            _same(got, ref)
    finally:
        job.close()
    return ref


@pytest.fixture(scope="module")
def cfg2_20k():
    from adam_amd import synth
    return synth.config_batch("cfg2", 20000)


def test_cfg2_first_reads(cfg2_20k):
    _three_ways(cfg2_20k)


def test_mixed_lengths():
    from adam_amd import bqsr, synth
    with bqsr.Context.get(0).tuned(order="read"):
        _three_ways(synth.generate(3000, (16, 37, 100, 150), 1, seed=63))


def test_chars_above_0xff():
    # chars above 0xFF need error rates no read produces (mismatches beyond the
    # observations): the crafted table of test_gpu_parity_more replaces the
    # observed one between the observe stage and the tail, in every mode
    from test_gpu_parity_more import crafted_table, reads_for_keys
    from adam_amd import _capi, bqsr
    d, w, keys = crafted_table(7)
    batch = reads_for_keys(keys, 3000, 7)

    def step(job):
        import torch
        L, ctx, bh, th, sp = job.L, job.ctx.handle, job.bh, job.th, job.sp
        _capi.check(L.bqsr_job_reset_async(bh, th, sp))
        _capi.check(L.bqsr_observe_stage(ctx, bh, job.sites_h, th, _capi.STAGE_PREP, sp))
        _capi.check(L.bqsr_observe_stage(ctx, bh, job.sites_h, th, _capi.STAGE_KERNEL | _capi.STAGE_FORK, sp))
        job.table.copy_(torch.from_numpy(w).to(job.dev))
        ptr = job._ptr
        _capi.check(L.bqsr_job_tail_async(ctx, bh, job.sites_h, th, ctypes.byref(job.lut), ptr(job.out_qual),
                                          ptr(job.out_start), ptr(job.out_len), ptr(job.exc), job.max_exc, sp))
        em, nexc = ctypes.c_double(), ctypes.c_int64()
        st = L.bqsr_job_result(bh, job.lut, ctypes.byref(em), ctypes.byref(nexc), sp)
        job.tail_path = int(L.bqsr_job_tail_path(bh))
        job.n_exc = int(nexc.value)
        _capi.check(st)

    with bqsr.Context.get(0).tuned(order="read"):
        ref = _three_ways(batch, dims=_capi.Dims(2, 10), step=step)
    assert ref["n_exc"] > 100  # (the same count in mode 2: the redo resets it)


def test_apply_error_raised_once():
    # a read without MD whose key is in no table row: MISSING_KEY from apply,
    # the same first read in every mode; the redo resets the error word and the
    # exception count before it runs again
    from test_gpu_parity import rec
    from adam_amd.records import RecordBatch
    recs = [rec(), rec(mismatching_positions=None, qual="++++++++++"), rec(qual="HHHHHHHHHH")]
    ref = _three_ways(RecordBatch.from_records(recs * 50), expect_error=True)
    assert ref["n_exc"] == 0


@pytest.mark.parametrize("case", ["no_reads", "one_read", "all_filtered", "all_masked"])
def test_small_and_empty(case):
    from test_gpu_parity import rec
    from adam_amd import _capi
    from adam_amd.records import RecordBatch
    if case == "no_reads":  # nothing to speculate on: the serial schedule, EMPTY_TABLE from finalize
        b = RecordBatch.from_records([rec()]).slice(0, 0)
        _three_ways(b, dims=_capi.Dims(1, 10), expect_error=True, paths=(SERIAL, SERIAL, SERIAL))
    elif case == "one_read":
        _three_ways(RecordBatch.from_records([rec()]))
    elif case == "all_filtered":
        # no usable read: em = 0 and g_obs = 0, avg = 0 / 0 is NaN in both
        # versions and compares equal to itself; EMPTY_TABLE in every mode
        recs = [rec(read_mapped=False), rec(duplicate_read=True), rec(primary_alignment=False)]
        ref = _three_ways(RecordBatch.from_records(recs * 3), expect_error=True)
        assert np.isnan(np.frombuffer(ref["final"][0], np.float64)[0])
    else:
        # every observed base masked: g_obs = 0, avg = em / 0 = inf, and the
        # rows' a2 = e + (inf - inf) are NaN in both versions
        recs = [rec(cigar="10I", mismatching_positions="0"), rec(mismatching_positions=None)]
        ref = _three_ways(RecordBatch.from_records(recs))
        assert np.isinf(np.frombuffer(ref["final"][0], np.float64)[0])
        assert np.isnan(np.frombuffer(ref["a2"], np.float64)).any()


def test_consecutive_jobs_and_record_step(cfg2_20k):
    # one ResidentJob: speculative jobs back to back, with and without known
    # sites, then a record=True step (the serial stage calls) after them
    from adam_amd import bqsr, synth
    from adam_amd.job import ResidentJob
    b = cfg2_20k
    dims = bqsr.dims_of([b])
    snp = bqsr.SnpTable(synth.known_sites(2_000_000, seed=5))
    for table in (None, snp):
        job = ResidentJob(b, dims, table, 0)
        try:
            ref, err, path = _step(job, 0)
            assert path == SERIAL and err is None
            for mode, want in ((1, SPEC), (1, SPEC), (2, REDONE), (1, SPEC)):
                got, err, path = _step(job, mode)
                assert (path, err) == (want, None)
                _same(got, ref)
            got, err, path = _step(job, 1, lambda: job.step(True))
            assert (path, err) == (SERIAL, None)
            _same(got, ref)
            got, err, path = _step(job, 1)
            assert (path, err) == (SPEC, None)
            _same(got, ref)
        finally:
            job.close()


def _untouched_key_batch(b):
    """the batch with qual char 77, which occurs nowhere else, written at
    offsets 1 .. clip-1 of every read that starts with a soft clip of >= 3
    bases: its key is touched (masked bases count there) but never observed
    unmasked, so a2 = a1 = e + (v_g - avg) depends on expectedMismatch itself"""
    assert not (b.qual == 77).any()
    q = b.qual.copy()
    n = 0
    for r in range(b.n_reads):
        c0 = int(b.cigar[int(b.cigar_offset[r])]) if b.cigar_offset[r + 1] > b.cigar_offset[r] else 0
        if (c0 & 0xF) == 4 and (c0 >> 4) >= 3:  # BAM CIGAR word: S
            a = int(b.qual_offset[r])
            q[a + 1:a + (c0 >> 4)] = 77
            n += 1
    b.qual = q
    return n


def test_genuine_mismatch(cfg2_20k):
    import copy
    import oracle as O
    from adam_amd import bqsr
    from adam_amd.job import ResidentJob
    b = copy.deepcopy(cfg2_20k)
    assert _untouched_key_batch(b) == 168
    dims = bqsr.dims_of([b])
    # the input still exercises the path: on the CPU, em x 1.5 changes chars, em (1 + 2^-4) none
    od = O.Dims(dims.n_rg, dims.max_len)
    words, em = O.observe_mt(b, None, od, n_parts=1, nthreads=8, fold1=True)
    n = int(b.qual_offset[-1])
    out = {f: O.apply_mt(b, od, words, em * f, nthreads=8)[0][:n] for f in (1.0, 1.5, 1.0 + 2.0 ** -4)}
    assert (out[1.0] != out[1.5]).sum() == 1736
    assert (out[1.0] != out[1.0 + 2.0 ** -4]).sum() == 0
    job = ResidentJob(b, dims, None, 0)
    try:
        ref, err, path = _step(job, 0)
        assert (path, err) == (SERIAL, None)
        got, err, path = _step(job, 3)  # the compare kernel raised the redo word: apply ran again
        assert (path, err) == (REDONE, None)
        _same(got, ref)
        got, err, path = _step(job, 1)  # the true estimate is accepted on the same input
        assert (path, err) == (SPEC, None)
        _same(got, ref)
    finally:
        job.close()
