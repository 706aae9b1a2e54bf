"""The call-order contracts of the BQSR core's stage functions: what the
batch's state flags (prepped, prep_sites, chars_lut, tail_fork, obs_pending)
let through, refuse, and fall back to.  The stage functions and
bqsr_job_tail_async compose one set of launch helpers; these
tests pin which schedule a call sequence gets, and that every schedule leaves
the same bytes.

    1  KERNEL on a fresh batch                               INVALID_ARG
    2  PREP with known sites, KERNEL with sites=NULL          INVALID_ARG
    3  apply KERNEL | NO_LUT before a LUT stage of that LUT   INVALID_ARG
    5  KERNEL | FORK under spec_tail=1, then the serial FOLD / finalize /
       apply stages (a fork event nobody took): the results of spec_tail=0
       bit for bit, and the next tail on the batch speculates (path 1)
    6  the tail on a bucketed batch, and on a read-order batch with
       spec_tail=0: path 0, the bytes of the explicit stage calls
    7  an empty batch (0 reads) through the tail and through the explicit stage
       calls: EMPTY_TABLE from bqsr_job_result, path 0; its snapshot read part
       by part (bqsr_job_status_get): observe OK, finalize EMPTY_TABLE, apply OK
       (test_gpu_speculative_tail.test_small_and_empty[no_reads] asserts that
       the three spec_tail modes raise the same error, not which); and a batch
       whose one mapped read fails in observe and leaves the table empty:
       bqsr_job_result raises observe's error, the first in the reference's order

Asserted elsewhere, not repeated here:
    4  LUT, then KERNEL | NO_LUT leaves what one KERNEL stage leaves:
       test_gpu_speculative_tail.test_consecutive_jobs_and_record_step (its
       record=True step is those two calls, compared with the one-stage job)

The batches: 300 reads of 100 bases (every fold block of the device gets
few reads or none), and 2400, which is more than one prep workgroup's 2048.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[300, 2400])
def batch(request):
    from adam_amd import synth
    return synth.generate(request.param, (100,), 1, seed=29)


@pytest.fixture(scope="module")
def snp():
    from adam_amd import bqsr
    return bqsr.SnpTable({"chr20": np.arange(1000, 64_000_000, 997, dtype=np.int64)})


class _Job:
    """a ResidentJob on a batch laid out in `order`, closed with its stream drained"""

    def __init__(self, batch, snp=None, order="read", dims=None):
        self.args = (batch, snp, order, dims)

    def __enter__(self):
        from adam_amd import bqsr
        from adam_amd.job import ResidentJob
        batch, snp, order, dims = self.args
        with bqsr.Context.get(0).tuned(order=order):
            self.job = ResidentJob(batch, dims or bqsr.dims_of([batch]), snp, 0)
        return self.job

    def __exit__(self, *exc):
        self.job.torch.cuda.synchronize(self.job.dev)
        self.job.close()


def _observe(job, stages, sites="own"):
    return job.L.bqsr_observe_stage(job.ctx.handle, job.bh, job.sites_h if sites == "own" else sites, job.th, stages,
                                    job.sp)


def _apply(job, stages):
    p = job._ptr
    return job.L.bqsr_apply_stage(job.ctx.handle, job.bh, job.lut, p(job.out_qual), p(job.out_start), p(job.out_len),
                                  p(job.exc), job.max_exc, stages, job.sp)


def _stage_calls(job, fork=False):
    """one job by the explicit stage calls: reset, PREP, KERNEL (| FORK), FOLD, finalize, apply KERNEL"""
    from adam_amd import _capi
    _capi.check(job.L.bqsr_job_reset_async(job.bh, job.th, job.sp))
    _capi.check(_observe(job, _capi.STAGE_PREP))
    _capi.check(_observe(job, _capi.STAGE_KERNEL | (_capi.STAGE_FORK if fork else 0)))
    p = job._ptr
    job._serial_tail(False, lambda i: None, (p(job.out_qual), p(job.out_start), p(job.out_len), p(job.exc), job.max_exc))
    em, nexc = ctypes.c_double(), ctypes.c_int64()
    st = job.L.bqsr_job_result(job.bh, job.lut, ctypes.byref(em), ctypes.byref(nexc), job.sp)
    job.tail_path = int(job.L.bqsr_job_tail_path(job.bh))
    job.n_exc = int(nexc.value)
    _capi.check(st)


def test_kernel_before_prep(batch):
    from adam_amd import _capi
    with _Job(batch) as job:
        assert _observe(job, _capi.STAGE_KERNEL) == _capi.INVALID_ARG


def test_kernel_with_other_sites(batch, snp):
    from adam_amd import _capi
    with _Job(batch, snp) as job:
        assert job.sites_h
        _capi.check(_observe(job, _capi.STAGE_RESET | _capi.STAGE_PREP))
        assert _observe(job, _capi.STAGE_KERNEL, sites=None) == _capi.INVALID_ARG
        _capi.check(_observe(job, _capi.STAGE_KERNEL))  # with prep's sites the kernel runs


def test_apply_kernel_before_lut_stage(batch):
    from adam_amd import _capi
    with _Job(batch) as job:
        _capi.check(_observe(job, _capi.STAGE_RESET | _capi.STAGE_PREP | _capi.STAGE_KERNEL | _capi.STAGE_FOLD))
        em = ctypes.c_void_p(job.L.bqsr_batch_em_device_ptr(job.bh))
        _capi.check(job.L.bqsr_finalize_device(job.ctx.handle, job.th, em, ctypes.byref(job.lut), job.sp))
        assert _apply(job, _capi.STAGE_RESET | _capi.STAGE_KERNEL | _capi.STAGE_NO_LUT) == _capi.INVALID_ARG
        _capi.check(_apply(job, _capi.STAGE_LUT))
        _capi.check(_apply(job, _capi.STAGE_KERNEL | _capi.STAGE_NO_LUT))


def test_fork_nobody_took(batch):
    from test_gpu_speculative_tail import SERIAL, SPEC, _same, _step
    with _Job(batch) as job:
        ref, err, path = _step(job, 0)
        assert (path, err) == (SERIAL, None)
        got, err, path = _step(job, 1, lambda: _stage_calls(job, fork=True))
        assert (path, err) == (SERIAL, None)
        _same(got, ref)
        got, err, path = _step(job, 1)
        assert (path, err) == (SPEC, None)
        _same(got, ref)


@pytest.mark.parametrize("order,mode", [("group", 1), ("read", 0)])
def test_serial_tail_is_the_stage_calls(batch, order, mode):
    from test_gpu_speculative_tail import SERIAL, _same, _step
    with _Job(batch, order=order) as job:
        ref, err, path = _step(job, mode, lambda: _stage_calls(job))
        assert (path, err) == (SERIAL, None)
        got, err, path = _step(job, mode)  # ResidentJob.step: KERNEL | FORK, bqsr_job_tail_async
        assert (path, err) == (SERIAL, None)
        _same(got, ref)


def _parts(job):
    """the last job's snapshot read one part at a time: ([observe, finalize, apply] statuses, em, exception count)"""
    from adam_amd import _capi
    _capi.check(job.L.bqsr_job_status_async(job.bh, job.lut, 0, job.sp))
    job.torch.cuda.synchronize(job.dev)
    em, nexc = ctypes.c_double(-1.0), ctypes.c_int64(-1)
    st = [job.L.bqsr_job_status_get(job.bh, 0, part, ctypes.byref(em), ctypes.byref(nexc)) for part in range(3)]
    return st, em.value, nexc.value


def test_empty_batch_is_empty_table():
    from adam_amd import _capi, bqsr, synth
    batch = synth.generate(300, (100,), 1, seed=29)
    with _Job(batch.slice(0, 0), dims=bqsr.dims_of([batch])) as job:
        # the explicit stage calls, then ResidentJob.step (bqsr_job_tail_async, spec_tail=1: nothing to speculate on)
        for step in (lambda: _stage_calls(job), job.step):
            with pytest.raises(_capi.BQSRError) as e:
                step()
            assert e.value.status == _capi.EMPTY_TABLE
            assert job.tail_path == 0
            assert _parts(job) == ([0, _capi.EMPTY_TABLE, 0], 0.0, 0)


def test_observe_error_comes_before_empty_table():
    from test_gpu_parity import rec
    from adam_amd import _capi
    from adam_amd.records import RecordBatch
    batch = RecordBatch.from_records([rec(mismatching_positions="5Z4"), rec(read_mapped=False)])
    with _Job(batch) as job:
        for step in (lambda: _stage_calls(job), job.step):
            with pytest.raises(_capi.BQSRError) as e:
                step()
            assert (e.value.status, e.value.read) == (_capi.MD_PARSE, 0)
            assert _parts(job)[0][:2] == [_capi.MD_PARSE, _capi.EMPTY_TABLE]
