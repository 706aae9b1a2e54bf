"""What the eight ``bqsr_*_kernel_times`` calls report after real jobs: every
stage that ran is above 0 and the stages of a call fit inside the host wall
time around it, a job zeroes its own stages, a failing job keeps the stages
it finished, the values are per thread (per handle for compare), and
print_tags over Arrow chunks sums its chunks.  DESIGN.md §6 and
tools/bench_adam.py rest on these numbers."""
import ctypes
import math
import os
import threading
import time

import pytest

import _mpileup_gen as MG
import _pileup_gen as G
from adam_amd import _capi, aggregate_pileups as AP, bam_writer, bqsr
from adam_amd import compare as C
from adam_amd import mpileup as M
from adam_amd import parquet as P
from adam_amd import print_tags as PT
from adam_amd import reads2ref as R
from adam_amd import realignment_targets as RT
from adam_amd import sam as S
from adam_amd.sam import SamText

pytestmark = pytest.mark.gpu

SAM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_resources", "artificial.sam")
FORMS = ("sam", "bam", "adam")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """artificial.sam as SAM text, BAM bytes and an ADAM Parquet directory, and a header-only SAM file"""
    from adam_amd.transform import transform
    d = tmp_path_factory.mktemp("kernel_times")
    with open(SAM, "rb") as fh:
        data = fh.read()
    bam = str(d / "in.bam")
    with open(bam, "wb") as fh:
        fh.write(bam_writer.sam_to_bam(data))
    adam = str(d / "in.adam")
    transform(SAM, adam)
    empty = str(d / "empty.sam")
    with open(empty, "wb") as fh:
        fh.write(G.HEADER)
    return {"sam": SAM, "bam": bam, "adam": adam, "empty": empty, "dir": d}


def parse(path):
    return SamText.read(path)


def walled(call):
    """(what call() returned, the host wall time around it in ms)"""
    t0 = time.perf_counter()
    out = call()
    return out, (time.perf_counter() - t0) * 1e3


def ran(times, wall_ms, names=None):
    """every stage the call ran (`names`; default: all) is finite and above 0, and together they fit inside the
    wall time: each span lies inside the call"""
    times = dict(times) if isinstance(times, dict) else dict(enumerate(times))
    names = list(times) if names is None else names
    print("stages", times, "of the call", names, "wall_ms", wall_ms)
    for k in names:
        assert math.isfinite(times[k]) and times[k] > 0.0, (k, times)
    assert sum(times[k] for k in names) <= wall_ms, (times, wall_ms)


def zeros(times):
    v = list(times.values()) if isinstance(times, dict) else list(times)
    print("zeros", v)
    assert v and all(x == 0.0 for x in v), times


# ---- each stage that ran ---------------------------------------------------------

def arrow_reads(adam, columns, locus=True, **kw):
    t = P.read_table(adam, columns=columns)
    return P.ArrowReads(R.locus_filter(t) if locus else t, bqsr.Context.get(0), **kw)


@pytest.mark.parametrize("form", FORMS)
def test_reads2ref(inputs, form):
    A = arrow_reads(inputs["adam"], R.PROJECTION) if form == "adam" else parse(inputs[form])
    try:
        t, wall = walled(lambda: R.arrow_pileups(A) if form == "adam" else A.pileups())
        assert t.num_rows > 0
        ran(R.kernel_times(), wall)
    finally:
        A.close()


@pytest.mark.parametrize("form", FORMS)
def test_mpileup(inputs, form):
    A = arrow_reads(inputs["adam"], M.PROJECTION, markdup=True) if form == "adam" else parse(inputs[form])
    try:
        text, wall = walled(lambda: b"".join(M.arrow_mpileup(A) if form == "adam" else A.mpileup()))
        assert text
        assert list(M.kernel_times()) == list(M.KERNELS)
        ran(M.kernel_times(), wall)
    finally:
        A.close()


@pytest.mark.parametrize("form", FORMS)
def test_realignment_targets(inputs, form):
    A = arrow_reads(inputs["adam"], RT.PROJECTION, locus=False) if form == "adam" else parse(inputs[form])
    try:
        t, wall = walled(lambda: RT.arrow_targets(A) if form == "adam" else A.realignment_targets())
        assert len(t["target_start"]) > 0
        assert list(RT.kernel_times()) == list(RT.KERNELS)
        ran(RT.kernel_times(), wall)
    finally:
        A.close()


@pytest.mark.parametrize("form", FORMS)
def test_aggregate_pileups(inputs, form):
    st, wall = walled(lambda: AP.aggregate_pileups(inputs[form], str(inputs["dir"] / ("agg_" + form))))
    assert st["rows_out"] > 0
    assert list(st["kernel_ms"]) == ["keys", "sort", "scans", "emit"]
    assert AP.kernel_times() == st["kernel_ms"]
    ran(st["kernel_ms"], wall)


def test_print_tags_sam_and_bam(inputs):
    for form in ("sam", "bam"):
        s = parse(inputs[form])
        try:
            (tags, total), wall = walled(s.tag_counts)
            assert tags["AS"] == total == 10
            scan = PT.kernel_times()
            ran(scan, wall, names=[0])
            values, wall = walled(lambda: PT.sam_tag_values(s, "AS"))
            assert sum(values.values()) == 10
            after = PT.kernel_times()
            assert after[0] == scan[0]  # (a values call leaves the counts call's time)
            ran(after, wall, names=[1])
        finally:
            s.close()


def tag_chunks(adam, repeat=1):
    import pyarrow as pa
    t = P.read_table(adam, columns=PT.PROJECTION).combine_chunks()
    return PT.table_chunks(pa.concat_tables([t] * repeat))


def test_print_tags_arrow(inputs):
    chunks, keep = tag_chunks(inputs["adam"])
    (tags, total), wall = walled(lambda: PT.arrow_tag_counts(chunks))
    assert tags["AS"] == total == 10
    ran(PT.kernel_times(), wall, names=[0])
    values, wall = walled(lambda: PT.arrow_tag_values(chunks, "AS"))
    assert sum(values.values()) == 10
    ran(PT.kernel_times(), wall, names=[1])
    del keep


def test_bam_output_host_compressor(inputs):
    s = parse(inputs["sam"])
    try:
        rec, wall = walled(s.bam_records)
        assert len(rec) > 0 and S.bgzf_compress(rec)
        ran(S.bam_kernel_times(), wall)
    finally:
        s.close()


def test_bam_output_device_compressor(inputs):
    s = parse(inputs["sam"])
    try:
        members, wall = walled(s.bam_members)
        assert members
        ran(S.bam_kernel_times() + S.bgzf_deflate_times(), wall)
    finally:
        s.close()


def members_of(b):
    n = at = 0
    while at < len(b):
        assert b[at:at + 4] == b"\x1f\x8b\x08\x04"
        at += int.from_bytes(b[at + 16:at + 18], "little") + 1
        n += 1
    return n


def test_bgzf_deflate_two_members():
    data = bytes((i * 7 + i // 300) & 0xFF for i in range(70000))
    out, wall = walled(lambda: S.bgzf_deflate(data))
    assert members_of(out) == 2
    ran(S.bgzf_deflate_times(), wall)


def test_compare_with_itself(inputs):
    for form in FORMS:
        out, wall = walled(lambda: C.compare_device(inputs[form], inputs[form], C.COMPARISON_NAMES))
        assert out.stats["pairs"] > 0
        assert len(out.stats["kernel_ms"]) == 3
        ran(out.stats["kernel_ms"], wall)


# ---- zeroing ---------------------------------------------------------------------

def test_header_only_input_zeroes_every_stage(inputs):
    full, empty = parse(inputs["sam"]), parse(inputs["empty"])
    try:
        # reads2ref, mpileup, realignment targets and print_tags: a job with reads, then one without on the same thread
        full.pileups()
        assert min(R.kernel_times()) > 0.0
        assert empty.pileups().num_rows == 0
        zeros(R.kernel_times())
        assert b"".join(full.mpileup())
        assert min(M.kernel_times().values()) > 0.0
        assert b"".join(empty.mpileup()) == b""
        zeros(M.kernel_times())
        full.realignment_targets()
        assert min(RT.kernel_times().values()) > 0.0
        assert len(empty.realignment_targets()["target_start"]) == 0
        zeros(RT.kernel_times())
        full.tag_counts()
        PT.sam_tag_values(full, "AS")
        assert min(PT.kernel_times()) > 0.0
        assert empty.tag_counts() == ({}, 0)
        assert PT.sam_tag_values(empty, "AS") == {}
        zeros(PT.kernel_times())
    finally:
        full.close()
        empty.close()
    AP.aggregate_pileups(inputs["sam"], str(inputs["dir"] / "agg_full"))
    assert min(AP.kernel_times().values()) > 0.0
    st = AP.aggregate_pileups(inputs["empty"], str(inputs["dir"] / "agg_empty"))
    assert st["rows_in"] == 0
    zeros(st["kernel_ms"])
    zeros(AP.kernel_times())


def some(times):
    """finite and not below 0: what an empty span between two marks gives"""
    print("empty spans", times)
    assert all(math.isfinite(x) and x >= 0.0 for x in times), times


def test_header_only_input_where_the_marks_are_still_recorded(inputs):
    """BAM output and compare record their marks around no kernel when there is no read, so a header-only input
    gives an empty span's time (finite, not below 0), not the time of the job before it; what such an input
    never reaches is 0; and bqsr_bgzf_deflate of no bytes returns before it touches the thread's values"""
    full, empty = parse(inputs["sam"]), parse(inputs["empty"])
    try:
        full.bam_members()
        before = S.bam_kernel_times() + S.bgzf_deflate_times()
        assert min(before) > 0.0
        assert len(empty.bam_records()) == 0
        some(S.bam_kernel_times())
        assert S.bgzf_deflate_times() == before[2:]  # (bam_records runs no deflate)
        assert empty.bam_members() == b""
        len_ms, write_ms = S.bam_kernel_times()
        some([len_ms])
        assert write_ms == 0.0  # (no stream: the second pass does not run)
        zeros(S.bgzf_deflate_times())
        full.bam_members()
        before = S.bgzf_deflate_times()
        assert min(before) > 0.0
        assert S.bgzf_deflate(b"") == b""
        assert S.bgzf_deflate_times() == before
    finally:
        full.close()
        empty.close()
    out = C.compare_device(inputs["empty"], inputs["empty"], C.COMPARISON_NAMES)
    assert out.stats["pairs"] == 0
    some(out.stats["kernel_ms"])


def test_a_later_job_reports_its_own_values(inputs):
    """mpileup's text stage after a prepare of the next input is that prepare's 0, not the earlier window's time;
    BAM output's second pass after the next prepare likewise"""
    a, b = parse(inputs["sam"]), parse(inputs["sam"])
    try:
        assert b"".join(a.mpileup())
        first = M.kernel_times()
        assert first["text"] > 0.0
        M.sam_prepare(b)
        second = M.kernel_times()
        assert second["text"] == 0.0 and all(second[k] > 0.0 for k in M.KERNELS[:4])
        a.bam_records()
        assert min(S.bam_kernel_times()) > 0.0
        sz = S.BamSizes()
        _capi.check(b.L.bqsr_sam_bam_prepare(b.ctx.handle, b.h, 0, b.counts().n_reads, None, ctypes.byref(sz)))
        len_ms, write_ms = S.bam_kernel_times()
        assert len_ms > 0.0 and write_ms == 0.0
    finally:
        a.close()
        b.close()


# ---- a failing input -------------------------------------------------------------

def test_unsorted_mpileup_keeps_the_walk_time():
    text = MG.sam_text([(8, "5M"), (2, "5M")], seed=3)  # the second kept read starts before the first
    s = SamText(text)
    try:
        with pytest.raises(_capi.BQSRError) as e:
            b"".join(s.mpileup())
        assert e.value.status == _capi.UNSORTED and e.value.read == 1
        kt = M.kernel_times()
        print("unsorted", kt)
        assert kt["walk"] > 0.0
        assert [kt[k] for k in ("emit", "sort", "group", "text")] == [0.0] * 4
    finally:
        s.close()


# ---- per thread, per handle ------------------------------------------------------

def thread_local_times():
    return {"reads2ref": tuple(R.kernel_times()), "mpileup": tuple(M.kernel_times().values()),
            "realignment_targets": tuple(RT.kernel_times().values()),
            "aggregate_pileups": tuple(AP.kernel_times().values()), "print_tags": tuple(PT.kernel_times()),
            "bam": tuple(S.bam_kernel_times()), "deflate": tuple(S.bgzf_deflate_times())}


def test_a_thread_that_ran_no_job_sees_zeros(inputs):
    AP.aggregate_pileups(inputs["sam"], str(inputs["dir"] / "agg_thread"))  # (first: it prepares a reads2ref job)
    s = parse(inputs["sam"])
    try:
        s.pileups()
        assert b"".join(s.mpileup())
        s.realignment_targets()
        s.tag_counts()
        PT.sam_tag_values(s, "AS")
        s.bam_members()
    finally:
        s.close()
    mine = thread_local_times()
    for name, v in mine.items():
        assert min(v) > 0.0, (name, v)
    seen = {}
    t = threading.Thread(target=lambda: seen.update(thread_local_times()))
    t.start()
    t.join()
    assert set(seen) == set(mine)
    for name, v in seen.items():
        zeros(v)
    assert thread_local_times() == mine


def test_two_compare_handles_keep_separate_times(inputs):
    L = C._lib()
    ctx = bqsr.Context.get(0)
    opt = C._Options(hash_bits=64, comparisons=sum(C.CMP_BIT.values()))
    sides = [C._open_side(inputs["sam"], ctx, C.COMPARISON_NAMES) for _ in range(2)]
    h = [ctypes.c_void_p(), ctypes.c_void_p()]
    try:
        for x in h:
            _capi.check(L.bqsr_compare_create(ctx.handle, ctypes.byref(opt), ctypes.byref(x)))
        zeros(C._kernel_times(h[0]))
        res = C._Result()
        d1, d2 = sides[0].struct(), sides[1].struct()
        _capi.check(L.bqsr_compare_sides(h[0], ctypes.byref(d1), ctypes.byref(d2), (C._Term * 1)(), 0, None,
                                         ctypes.byref(res)))
        assert res.n_pairs > 0
        first = C._kernel_times(h[0])
        assert min(first) > 0.0
        zeros(C._kernel_times(h[1]))
        _capi.check(L.bqsr_compare_sides(h[1], ctypes.byref(d1), ctypes.byref(d2), (C._Term * 1)(), 0, None,
                                         ctypes.byref(res)))
        assert min(C._kernel_times(h[1])) > 0.0
        assert C._kernel_times(h[0]) == first
    finally:
        for x in h:
            if x:
                L.bqsr_compare_destroy(x)
        for s in sides:
            s.close()


# ---- Arrow print_tags sums its chunks ----------------------------------------------

def test_arrow_print_tags_sums_its_chunks(inputs):
    chunks, keep = tag_chunks(inputs["adam"], repeat=2)
    assert len(chunks) == 2
    PT.arrow_tag_counts(chunks)  # (the first launch of the kernel is not what is compared)
    alone = []
    for c in chunks:
        assert PT.arrow_tag_counts([c])[1] == 10
        alone.append(PT.kernel_times()[0])
    assert PT.arrow_tag_counts(chunks)[1] == 20
    both = PT.kernel_times()[0]
    print("scan alone", alone, "both", both)
    assert min(alone) > 0.0
    assert both >= max(alone)
    del keep
