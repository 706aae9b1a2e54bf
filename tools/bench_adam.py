"""End-to-end `transform IN.sam OUT.adam [-mark_duplicate_reads]
-recalibrate_base_qualities` throughput (§8 f2): synthetic cfg2-like reads as
SAM text (or BAM) in a file, the whole transform timed -- device parse,
MarkDuplicates, BQSR, ADAM columns on the device, Parquet part files written
by host threads -- and one JSON line printed with the phase split.

    python tools/bench_adam.py --reads 10000000 [--bam] [--no-markdup] [--sort_reads]
        [--compression none|snappy|gzip] [--part-reads N] [--partition-bytes B]

--sort_reads adds `-sort_reads` (the "sort" phase in the stats' phase split)
and prints record_text_bytes: the gather kernel (sort_gather) moves twice that.

    python tools/bench_adam.py --flagstat [--reads 2000000] [--kernel-reads 64000000] [--reps 5]

--flagstat measures `adam flagstat` (adam_amd/flagstat.py) instead: over the
same synthetic reads as SAM, as BAM and as their ADAM Parquet, the parse and
the flagstat call (host clock around calls that end in a synchronise; the
best of --reps), Arrow's read, the upload-and-count call and the kernel alone
(device events, buffers resident); then the Arrow-form kernel alone over
--kernel-reads random reads on the device, as bytes/s.  One JSON line.

    python tools/bench_adam.py --reads2ref [--reads 2000000] [--part-reads N] [--compression snappy]
    python tools/bench_adam.py --reads2ref --parquet-encoder [--reads 2000000]   (host next to device pages)
    python tools/bench_adam.py [--reads2ref] --parquet-encoder --device-snappy-only   (device pages under snappy:
                                                 -parquet_compressor host next to device, nothing else)

--reads2ref measures `adam reads2ref` (adam_amd/reads2ref.py) over the same
synthetic reads as SAM text: the job's steps run one after the other in the
main thread, each timed by the host clock around calls that end in a
synchronise -- parse, count (bqsr_sam_pileup_prepare), emit + D2H
(bqsr_sam_pileup_columns: the kernel by device events, the copies as the
rest of the call), the read-level columns and the Arrow table -- while the
writer's host threads encode the part files behind it (their busy seconds
summed; `close` is the wait for them at the end).  The two kernels' times are
device events; the emit kernel's bytes written per second stand beside the
copy rate DESIGN.md uses.  One JSON line.

    python tools/bench_adam.py --aggregate [--reads 2000000] [--restatement-reads 200000]

--aggregate measures `adam aggregate_pileups` (adam_amd/aggregate_pileups.py)
over the same synthetic reads as --reads2ref, read input (the rows never leave
the device), next to the unaggregated `reads2ref` job on the same file: both
legs in this process, each run once after a warm-up run of its own.  Per leg
the end-to-end seconds, rows in and out and the phase split (host clock); for
the aggregation the device-event ms of its keys, sort, scans and emit stages;
and the single-threaded Python restatement (tests/_pileup_ref.py,
tests/_pileup_agg_ref.py) on the first --restatement-reads reads, whose result
the command's on the same reads must equal.  One JSON line.

    python tools/bench_adam.py --bam-out [--reads 2000000] [--bam-level 6]

--bam-out measures `transform IN.sam OUT.bam` (transform._BamOut) next to
`transform IN.sam OUT.sam` over the same input in the same run (both warmed,
the best of --reps): MarkDuplicates and BQSR over synthetic reads generated
without Q <= 2 read ends (BAM refuses the reference's trimmed recalibrated
strings; should a recalibrated char still leave '!'..'~' the refusal is
reported and both legs rerun without BQSR).  Reads/s and the phase split of
both legs, the two encoder kernels by device events with the bytes they move
(pass 1 reads the record text; pass 2 reads it again and writes the records)
as a fraction of 8 TB/s, and the compressor's MB/s of stream.  Then, in the
same run, the BAM leg again with the host compressor at level 1 and with the
device compressor (-bam_compressor device: the deflate and pack kernels'
device-event ms, GB/s of stream, the bytes downloaded, the file's size);
every leg's --reps timed runs are all reported (seconds_all) with their
spread.  One JSON line.

    python tools/bench_adam.py --bam-out --bam-index [--reads 2000000] [--bam-level 6]

--bam-region measures `python -m adam_amd.bam_index OUT.bam` (the index of an
existing BAM, built from windows of the file: bam_windows.hip) next to the
index stages of `transform -bam_index` on the same reads and next to
tests/_bai_ref.bai_of_bam on the same file, and `flagstat OUT.bam -region R`
(R holds about 1 % of the reads, read through the index) next to `flagstat
OUT.bam`: the 2M reads sorted by position, all legs in one process, warmed,
three timed runs each, alternating; medians and spreads.

--bam-out --bam-index measures `transform IN.sam OUT.bam -bam_index`
(transform._BamOut, bam_index.hip) over the same synthetic reads sorted by
position on the host, MarkDuplicates, no BQSR: with the host compressor at
--bam-level and with the device compressor, a leg without the index and a leg
with it, all in this process, three timed runs each after a warm-up (all
reported, with their spread).  Per index leg the stages by device events, the
host's member walk and serialisation by the host clock, the index's bytes and
chunk and bin counts; then tests/_bai_ref.bai_of_bam on the finished file --
the external pass the flag replaces -- timed, its bytes required to equal the
device's.  On a tree whose transform has no bam_index argument the no-index
legs alone are run: the same tool measures the parent commit.  One JSON line.

    python tools/bench_adam.py --adam2sam [--reads 2000000] [--bam-level 6]

--adam2sam measures `adam2sam` (adam_amd/adam2sam.py): the synthetic reads
written once as .adam (--compression), then in this process, three timed runs
each after a warm-up (all reported, with their spread), ADAM -> SAM and ADAM ->
BAM (host compressor at --bam-level, and the device compressor) next to
`transform` SAM -> SAM and SAM -> BAM over the same reads (no MarkDuplicates, no
BQSR: the same sinks).  Per adam2sam leg the phase split -- Arrow's Parquet
read on the host, the header synthesis, the chunk buffers, their upload, the
two line kernels by device events (per byte of record text too), the parse,
emit, close.  The same reads are parsed once more as BAM input, whose lines
bam_lines_len / bam_lines_write render: a rocprofv3 --kernel-trace --stats run
of this leg puts the two pairs of kernels side by side.  One JSON line.

    python tools/bench_adam.py --print-tags [--reads 2000000] [--variant-lib LIB.so]

--mpileup measures `adam mpileup` (adam_amd/mpileup.py) over the same
synthetic reads after `transform -sort_reads`.  The generator draws every
read's bases and MD on its own, so overlapping reads disagree on the reference
base, which mpileup refuses as the reference asserts: of the reads
LocusPredicate keeps, those that overlap the kept read before them are left
out.  Once each after a warm-up, in this process: mpileup and reads2ref on
that file (end-to-end seconds, phase split, mpileup's stages by device
events), then the single-threaded Python restatement (tests/_mpileup_ref.py)
on the first --restatement-reads reads, whose text the command must equal.
One JSON line.

    python tools/bench_adam.py --mpileup [--reads 2000000]

--realign-targets measures the indel realignment targets
(adam_amd/realignment_targets.py) over the same synthetic reads as SAM text, as
generated (no sort, no filter: the finder takes every read).  Once after a
warm-up, in this process: the command end to end (phase split by the host
clock, the stages by device events, the fold by the host clock), then, on the
same file, reads2ref's prepare (the pileup walk alone) and `adam mpileup`
(which refuses unsorted reads or reads that disagree on the reference base:
its seconds or its refusal is reported), then the single-threaded Python
restatement (tests/_realign_targets_ref.py) on the first --restatement-reads
reads, whose arrays the device must equal.  One JSON line.

    python tools/bench_adam.py --realign-targets [--reads 2000000] [--restatement-reads 20000]

--print-tags measures `adam print_tags` (adam_amd/print_tags.py) over the same
synthetic reads as SAM text with aligner-like fields appended to every line
(NM:i, AS:i, XS:i, and XA:Z on about 5 % of the lines; samgen alone writes MD
and RG): once each, in this process, print_tags without -count, print_tags
-count NM,XA, flagstat on the same file (the yardstick: both are one parse
plus one pass over each record) and the single-threaded Python restatement
(tests/_tags_ref.py) on the first 200 000 reads; end-to-end seconds with the
phase split, the scan kernel's and the value kernels' device-event ms and the
bytes of record text the scan covers.  --variant-lib names a build of the
library with the other histogram form (tools/variants/tags_hist_plain.diff):
the scan kernel alone is then timed (best of --reps, device events, one parse)
by a child process per library, three times each, alternating, and both
forms' ms are reported.  One JSON line.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


CHUNK = 500_000


def log(msg):
    print("[bench_adam] " + msg, file=sys.stderr, flush=True)


def _chunk(args):
    from adam_amd import synth
    from adam_amd.samgen import sam_text
    r0, n, read_len, total = args[:4]
    kw = {"p_q2tail": args[4]} if len(args) > 4 else {}
    b = synth.generate(n, (read_len,), 2, 20261015 + 2, first_read=r0, **kw)
    text = sam_text(b, n_rg=2, qname="c%d_" % (r0 // CHUNK))
    if r0:  # the header once
        text = b"".join(l + b"\n" for l in text.split(b"\n") if l and not l.startswith(b"@"))
    return text


def synthetic_sam(n_reads: int, read_len: int, p_q2tail=None) -> bytes:
    """cfg2-like reads as SAM text, generated in slices by a process pool
    (before the GPU is touched); QNAMEs unique per read.  p_q2tail: the share
    of reads with a Q2 tail (None: the generator's default)"""
    from multiprocessing import get_context
    extra = () if p_q2tail is None else (p_q2tail,)
    jobs = [(r0, min(CHUNK, n_reads - r0), read_len, n_reads) + extra for r0 in range(0, n_reads, CHUNK)]
    # close() + join(), not the context manager: its terminate() SIGTERMs
    # workers still unwinding (under rocprofv3 the signal handler prints an
    # abort trace)
    pool = get_context("fork").Pool(min(16, max(1, len(jobs)), os.cpu_count() or 1))
    try:
        parts = []
        for i, t in enumerate(pool.imap(_chunk, jobs)):
            parts.append(t)
            log("slice %d / %d" % (i + 1, len(jobs)))
        pool.close()
    except BaseException:
        pool.terminate()
        raise
    finally:
        pool.join()
    return b"".join(parts)


def _ms(f, reps):
    """best wall time of f() in ms over reps calls (f ends in a device synchronise), and its last result"""
    best, r = None, None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = f()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best, r


def _kernel_ms(ctx, chunk, reps):
    """flagstat_arrow alone over device buffers: device events around `reps`
    launches (after a warm-up launch), ms per launch; the counters of one launch"""
    import ctypes

    import torch
    from adam_amd import flagstat as FS
    from adam_amd._capi import check
    L = FS._lib()
    counters = torch.zeros(37, dtype=torch.int64, device="cuda")
    counters[36] = -1
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(L.bqsr_flagstat_arrow_device(ctx.handle, ctypes.byref(chunk), counters.data_ptr(), sp))
    torch.cuda.synchronize()
    one = counters.cpu().numpy().copy()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        check(L.bqsr_flagstat_arrow_device(ctx.handle, ctypes.byref(chunk), counters.data_ptr(), sp))
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, one


def _device_chunk(table_or_n, seed=3):
    """a bqsr_flagstat_chunk of device buffers (bitmaps as whole 64-bit
    words): an Arrow table's columns, or n random reads (no read with a null
    mapq).  Returns (chunk, keep, bytes the kernel reads)."""
    import numpy as np
    import torch
    from adam_amd import flagstat as FS
    keep = []
    C = FS.FlagStatChunk()

    def dev(t):
        keep.append(t.cuda())
        return keep[-1].data_ptr()
    if isinstance(table_or_n, int):
        n = table_or_n
        W = (n + 63) // 64
        g = torch.Generator(device="cuda").manual_seed(seed)

        def rnd():  # 64 random bits a word
            hi, lo = (torch.randint(0, 1 << 32, (W,), dtype=torch.int64, device="cuda", generator=g) for _ in "hl")
            return (hi << 32) | lo
        for k in range(9):
            keep.append(rnd())
            C.bools[k] = keep[-1].data_ptr()
            keep.append(rnd() | rnd())
            C.bools_validity[k] = keep[-1].data_ptr()
        for attr, hi, valid in (("reference_id", 24, rnd() | rnd()), ("mate_reference_id", 24, rnd() | rnd()),
                                ("mapq", 61, torch.full((W,), -1, dtype=torch.int64, device="cuda"))):
            keep.append(torch.randint(0, hi, (n,), dtype=torch.int32, device="cuda", generator=g))
            setattr(C, attr, keep[-1].data_ptr())
            keep.append(valid)
            setattr(C, attr + "_validity", keep[-1].data_ptr())
        n_maps = 21
    else:
        import pyarrow as pa
        t = table_or_n.combine_chunks()
        n = t.num_rows
        n_maps = 0

        def words(buf):  # an Arrow bitmap as whole 64-bit words
            a = np.zeros(((n + 63) // 64) * 8, np.uint8)
            a[:(n + 7) // 8] = np.frombuffer(buf, np.uint8, (n + 7) // 8)
            return torch.from_numpy(a.view(np.int64))
        for k, name in enumerate(FS.BOOL_COLUMNS):
            if name not in t.column_names:
                continue
            b = pa.concat_arrays([t.column(name).chunk(0)]).buffers() if n else [None, None]
            C.bools[k] = dev(words(b[1]))
            n_maps += 1
            if b[0] is not None:
                C.bools_validity[k] = dev(words(b[0]))
                n_maps += 1
        for name, attr in zip(FS.INT_COLUMNS, ("reference_id", "mate_reference_id", "mapq")):
            if name not in t.column_names:
                continue
            arr = pa.concat_arrays([t.column(name).chunk(0).cast(pa.int32())])
            b = arr.buffers()
            setattr(C, attr, dev(torch.from_numpy(np.frombuffer(b[1], np.int32, n).copy())))
            if b[0] is not None:
                setattr(C, attr + "_validity", dev(words(b[0])))
                n_maps += 1
    C.n_reads = n
    n_int = sum(1 for a in ("reference_id", "mate_reference_id", "mapq") if getattr(C, a))
    return C, keep, n * 4 * n_int + ((n + 63) // 64) * 8 * n_maps


def bench_flagstat(a):
    """the --flagstat measurements (see the module doc)"""
    import torch
    from adam_amd import bqsr
    from adam_amd import flagstat as FS
    from adam_amd import parquet as P
    from adam_amd import transform as T
    from adam_amd.bam_writer import sam_to_bam_parallel
    from adam_amd.sam import SamText
    t0 = time.perf_counter()
    sam = synthetic_sam(a.reads, a.len)
    bam = sam_to_bam_parallel(sam, min(16, os.cpu_count() or 1))
    log("generated %d bytes of SAM, %d of BAM in %.1f s" % (len(sam), len(bam), time.perf_counter() - t0))
    torch.zeros(1, device="cuda")
    ctx = bqsr.Context.get(0)
    ctx.tune(bgzf=a.bgzf)
    reps = max(2, a.reps)
    res = {"metric": "adam flagstat: ms per phase at --reads (host clock, best of reps); Arrow-form kernel alone "
                     "at --kernel-reads (device events)",
           "reads": a.reads, "read_len": a.len, "reps": reps}
    counts = {}
    for name, data, is_bam in (("sam", sam, False), ("bam", bam, True)):
        parse_ms, st = _ms(lambda: SamText(data, ctx, bam=is_bam), 1)  # warm-up (and the handle that is counted)
        try:
            _ms(st.flagstat, 1)
            fs_ms, c = _ms(st.flagstat, reps)
        finally:
            st.close()

        def parse():
            SamText(data, ctx, bam=is_bam).close()
        parse_ms, _ = _ms(parse, reps)
        counts[name] = c
        res[name] = {"input_bytes": len(data), "parse_ms": parse_ms, "flagstat_ms": fs_ms}
        log("%s: parse %.2f ms, flagstat %.3f ms" % (name, parse_ms, fs_ms))
    work = a.dir or tempfile.mkdtemp(prefix="bench_flagstat_")
    os.makedirs(work, exist_ok=True)
    try:
        src, out = os.path.join(work, "in.sam"), os.path.join(work, "out.adam")
        with open(src, "wb") as fh:
            fh.write(sam)
        del sam, bam
        T.transform(src, out, compression=a.compression, part_reads=a.part_reads, overwrite=True)

        def read():
            t = P.read_table(out, columns=FS.PROJECTION)
            return t, FS.table_chunks(t)
        _ms(read, 1)
        read_ms, (table, (chunks, keep)) = _ms(read, reps)
        _ms(lambda: FS.arrow_flagstat(chunks, ctx), 1)
        call_ms, c = _ms(lambda: FS.arrow_flagstat(chunks, ctx), reps)
        counts["adam"] = c
        C, dkeep, nbytes = _device_chunk(table)
        k_ms, _ = _kernel_ms(ctx, C, 50)
        res["adam"] = {"input_bytes": sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out)),
                       "compression": a.compression, "record_batches": len(chunks), "arrow_read_ms": read_ms,
                       "upload_and_kernel_ms": call_ms, "kernel_ms": k_ms, "upload_ms": call_ms - k_ms,
                       "kernel_bytes": nbytes}
        log("adam: read %.2f ms, upload + kernel %.3f ms, kernel %.4f ms" % (read_ms, call_ms, k_ms))
        del dkeep, keep
    finally:
        if not a.dir:
            shutil.rmtree(work, ignore_errors=True)
    if not (counts["sam"] == counts["bam"] == counts["adam"]) or sum(x.total for x in counts["sam"]) != a.reads:
        raise SystemExit("flagstat differs between SAM, BAM and ADAM: %r" % (counts,))
    res["counts"] = {"failed": list(counts["sam"][0].counts()), "passed": list(counts["sam"][1].counts())}
    # the Arrow-form kernel alone
    C, dkeep, nbytes = _device_chunk(int(a.kernel_reads))
    k_ms, one = _kernel_ms(ctx, C, 20)
    if int(one[0]) + int(one[18]) != a.kernel_reads:
        raise SystemExit("kernel counted %d reads of %d" % (int(one[0]) + int(one[18]), a.kernel_reads))
    res["kernel"] = {"reads": int(a.kernel_reads), "bytes": nbytes, "ms": k_ms, "bytes_per_s": nbytes / (k_ms * 1e-3),
                     "copy_rate_bytes_per_s": 6.29e12, "share_of_copy_rate": nbytes / (k_ms * 1e-3) / 6.29e12,
                     "launches_timed": 20}
    log("kernel: %d reads, %d bytes, %.4f ms" % (a.kernel_reads, nbytes, k_ms))
    print(json.dumps(res))


def _tagged_sam(sam: bytes) -> bytes:
    """aligner-like optional fields appended to every record line"""
    out = []
    i = 0
    for l in sam.split(b"\n"):
        if not l:
            continue
        if l[:1] != b"@":
            h = (i * 2654435761) & 0xFFFFFFFF
            l += b"\tNM:i:%d\tAS:i:%d\tXS:i:%d" % (h % 7, 100 - h % 31, (h >> 8) % 90)
            if h % 20 == 0:
                l += b"\tXA:Z:chr%d,+%d,100M,%d;" % (1 + h % 22, 1 + (h >> 4) % 100000, h % 4)
            i += 1
        out.append(l)
    return b"\n".join(out) + b"\n"


def _scan_only(path, reps):
    """the scan kernel alone over one parse of `path`: best device-event ms of reps calls"""
    import torch
    from adam_amd import bqsr
    from adam_amd import print_tags as PT
    from adam_amd.sam import SamText
    torch.zeros(1, device="cuda")
    with open(path, "rb") as fh:
        st = SamText(fh.read(), bqsr.Context.get(0))
    try:
        st.tag_counts()
        best = None
        for _ in range(reps):
            st.tag_counts()
            ms = PT.kernel_times()[0]
            best = ms if best is None else min(best, ms)
    finally:
        st.close()
    return best


def bench_print_tags(a):
    """the --print-tags measurements (see the module doc)"""
    import subprocess
    if a.scan_only:  # the child of a --variant-lib run
        print(json.dumps({"scan_ms": _scan_only(a.scan_only, max(3, a.reps))}))
        return
    import torch
    from adam_amd import _capi, bqsr
    from adam_amd import flagstat as FS
    from adam_amd import print_tags as PT
    from adam_amd import transform as T
    t0 = time.perf_counter()
    sam = _tagged_sam(synthetic_sam(a.reads, a.len))
    header = T.sam_partitions(sam, len(sam))[0]
    log("generated %d bytes of SAM in %.1f s" % (len(sam), time.perf_counter() - t0))
    work = a.dir or tempfile.mkdtemp(prefix="bench_print_tags_")
    os.makedirs(work, exist_ok=True)
    res = {"metric": "adam print_tags at --reads: end-to-end seconds (host clock, one run each after a warm-up on a "
                     "small file), kernels by device events", "reads": a.reads, "read_len": a.len,
           "input_bytes": len(sam), "record_text_bytes": len(sam) - len(header)}
    try:
        src, small = os.path.join(work, "in.sam"), os.path.join(work, "small.sam")
        with open(src, "wb") as fh:
            fh.write(sam)
        n_small = min(a.reads, 200_000)
        cut = len(header)
        for _ in range(n_small):
            cut = sam.index(b"\n", cut) + 1
        with open(small, "wb") as fh:
            fh.write(sam[:cut])
        del sam
        torch.zeros(1, device="cuda")
        bqsr.Context.get(0)
        # warm-up: the context, the kernels' code objects, pyarrow
        PT._run(small, None, ("NM", "XA"), 0, a.partition_bytes)
        FS._flagstat(small, 0, a.partition_bytes)

        def run(f):
            t = time.perf_counter()
            r = f()
            return time.perf_counter() - t, r
        s1, r1 = run(lambda: PT._run(src, None, (), 0, a.partition_bytes))
        s2, r2 = run(lambda: PT._run(src, None, ("NM", "XA"), 0, a.partition_bytes))
        s3, r3 = run(lambda: FS._flagstat(src, 0, a.partition_bytes))
        if r1[3] != a.reads or r1[1] != r2[1] or sum(r2[2]["NM"].values()) != a.reads:
            raise SystemExit("print_tags counted %r of %d reads" % (r1[3], a.reads))
        res["print_tags"] = {"seconds": s1, "phases_s": r1[4]["phases"], "scan_kernel_ms": r1[4]["kernel_ms"]["scan"]}
        res["print_tags_count_NM_XA"] = {"seconds": s2, "phases_s": r2[4]["phases"],
                                         "scan_kernel_ms": r2[4]["kernel_ms"]["scan"],
                                         "value_kernels_ms": r2[4]["kernel_ms"]["values"],
                                         "distinct_values": {t: len(v) for t, v in r2[2].items()}}
        res["flagstat"] = {"seconds": s3, "phases_s": r3[2]["phases"]}
        res["print_tags_over_flagstat"] = s1 / s3
        res["tags"] = r1[1]
        # the restatement, single-threaded, on the first 200 000 reads
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from _adam_ref import convert_sam
        from _tags_ref import characterize_tags, sam_records
        with open(small, "rb") as fh:
            text = fh.read()
        s4, want = run(lambda: characterize_tags(sam_records(convert_sam(text))))
        got = PT._run(small, None, (), 0, a.partition_bytes)
        if (got[1], got[3]) != want:
            raise SystemExit("print_tags differs from the restatement on %d reads" % n_small)
        res["python_restatement"] = {"reads": n_small, "seconds": s4}
        log("print_tags %.3f s, -count NM,XA %.3f s, flagstat %.3f s, restatement (%d reads) %.1f s"
            % (s1, s2, s3, n_small, s4))
        if a.variant_lib:  # the scan kernel alone, a child process per library, the two alternating
            libs = (("leader_loop", _capi.LIB_PATH), ("plain_lds_atomics", os.path.abspath(a.variant_lib)))
            runs = {name: [] for name, _ in libs}
            for _ in range(3):
                for name, lib in libs:
                    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--print-tags", "--scan-only",
                                          src, "--reps", str(max(3, a.reps))],
                                         env=dict(os.environ, ADAM_BQSR_LIB=lib), check=True, capture_output=True,
                                         text=True).stdout
                    runs[name].append(json.loads(out.strip().splitlines()[-1])["scan_ms"])
                    log("%s: scan %.4f ms" % (name, runs[name][-1]))
            forms = {name: {"best_ms": min(v), "runs_ms": v} for name, v in runs.items()}
            res["histogram_forms_scan_ms"] = forms
    finally:
        if not a.dir:
            shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(res))


def bench_reads2ref(a):
    """the --reads2ref measurements (see the module doc)"""
    import ctypes
    import threading
    import torch
    from adam_amd import adam_save, bqsr
    from adam_amd import reads2ref as R
    from adam_amd._capi import check
    from adam_amd.sam import SamText
    t0 = time.perf_counter()
    sam = synthetic_sam(a.reads, a.len)
    log("generated %d bytes of SAM in %.1f s" % (len(sam), time.perf_counter() - t0))
    torch.zeros(1, device="cuda")
    ctx = bqsr.Context.get(0)
    L = R._lib()
    work = a.dir or tempfile.mkdtemp(prefix="bench_reads2ref_")
    os.makedirs(work, exist_ok=True)
    part_reads = a.part_reads if a.part_reads != 1 << 19 else R.DEFAULT_PART_READS
    ROW_BYTES = 3 * 8 + 7 * 4 + 2  # the device columns of one row; four validity bits on top

    def run(out):
        ph = {k: 0.0 for k in ("parse", "count", "count_kernel", "columns", "emit_kernel", "host_buffers",
                               "read_level_and_table", "add", "close")}
        busy = [0.0]
        lock = threading.Lock()
        t_all = time.perf_counter()
        W = adam_save.AdamWriter(out, a.compression, overwrite=True, dict_cols=adam_save.PILEUP_DICT_COLS,
                                 stats_cols=adam_save.PILEUP_STATS_COLS, huffman_cols=(), max_pending=2)
        write = W._write

        def timed_write(table, name):
            t = time.perf_counter()
            write(table, name)
            with lock:
                busy[0] += time.perf_counter() - t
        W._write = timed_write
        rows = 0
        ok = False
        try:
            t = time.perf_counter()
            st = SamText(sam, ctx)
            ph["parse"] += time.perf_counter() - t
            try:
                hdr = adam_save.header_info(st)
                n = st.counts().n_reads
                for r0 in range(0, n, part_reads):
                    m = min(part_reads, n - r0)
                    sz = R.PileupSizes()
                    t = time.perf_counter()
                    check(L.bqsr_sam_pileup_prepare(ctx.handle, st.h, r0, m, None, ctypes.byref(sz)))
                    ph["count"] += time.perf_counter() - t
                    ph["count_kernel"] += R.kernel_times()[0] * 1e-3
                    t = time.perf_counter()
                    H, arrays = R._host_columns(sz.n_rows)
                    ph["host_buffers"] += time.perf_counter() - t
                    t = time.perf_counter()
                    check(L.bqsr_sam_pileup_columns(ctx.handle, st.h, ctypes.byref(H), None))
                    ph["columns"] += time.perf_counter() - t
                    ph["emit_kernel"] += R.kernel_times()[1] * 1e-3
                    t = time.perf_counter()
                    table = R._table(sz.n_rows, arrays, R._sam_read_level(st, r0, m, hdr))
                    ph["read_level_and_table"] += time.perf_counter() - t
                    rows += sz.n_rows
                    t = time.perf_counter()
                    W.add(table)
                    ph["add"] += time.perf_counter() - t
                    del table, arrays, H
            finally:
                st.close()
            ok = True
        finally:
            t = time.perf_counter()
            W.close(ok)
            ph["close"] += time.perf_counter() - t
        return time.perf_counter() - t_all, rows, ph, busy[0], W.parts

    try:
        out = os.path.join(work, "out.adam")
        log("warm-up run")
        run(out)
        best = None
        for _ in range(max(1, a.reps)):
            log("timed run")
            r = run(out)
            if best is None or r[0] < best[0]:
                best = r
        dt, rows, ph, busy, parts = best
        out_bytes = sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out))
    finally:
        if not a.dir:
            shutil.rmtree(work, ignore_errors=True)
    emit_bytes = rows * ROW_BYTES + 4 * ((rows + 63) // 64) * 8
    d2h = ph["columns"] - ph["emit_kernel"]
    res = {"metric": "adam reads2ref SAM -> ADAMPileup Parquet: seconds per phase (host clock around synchronising "
                     "calls, main thread), the two kernels by device events, writer threads' busy seconds",
           "reads": a.reads, "read_len": a.len, "rows": rows, "input_bytes": len(sam), "output_bytes": out_bytes,
           "compression": a.compression, "part_reads": part_reads, "parts": parts, "seconds": dt,
           "rows_per_s": rows / dt, "reads_per_s": a.reads / dt,
           "phases_s": {"parse": ph["parse"], "count": ph["count"], "emit": ph["emit_kernel"], "d2h": d2h,
                        "host_buffers": ph["host_buffers"], "read_level_and_table": ph["read_level_and_table"],
                        "add_waiting_for_writers": ph["add"], "close": ph["close"]},
           "parquet_encode_busy_s": busy,
           "kernels": {"count_ms": ph["count_kernel"] * 1e3, "emit_ms": ph["emit_kernel"] * 1e3,
                       "emit_bytes_written": emit_bytes,
                       "emit_bytes_per_s": emit_bytes / ph["emit_kernel"] if ph["emit_kernel"] else None,
                       "copy_rate_bytes_per_s": 6.29e12,
                       "share_of_copy_rate": emit_bytes / ph["emit_kernel"] / 6.29e12 if ph["emit_kernel"] else None,
                       "count_reads_per_s": a.reads / ph["count_kernel"] if ph["count_kernel"] else None},
           "d2h_bytes": emit_bytes, "d2h_bytes_per_s": emit_bytes / d2h if d2h > 0 else None}
    log("%.2f s, %d rows, emit %.3f ms, count %.3f ms" % (dt, rows, ph["emit_kernel"] * 1e3, ph["count_kernel"] * 1e3))
    print(json.dumps(res))


def _device_snappy_legs(run, file_bytes, stats_of):
    """The device encoder under snappy with the host codec and with
    -parquet_compressor device, in this process on the same input: a warm-up
    each, then three timed runs each, the two legs alternating.  run(compressor)
    does one job and returns its statistics; file_bytes() the part files' bytes
    of the job just done; stats_of(st) -> (page kernels' ms, bytes downloaded).
    Per leg: the three wall times, their median and spread, the median run's
    phases, kernel times (the compressor's two among them) and bytes
    downloaded, the files' bytes; then the comparison, and whether the
    difference of the medians exceeds the larger of the two spreads."""
    legs = {"host": [], "device": []}
    sizes = {}
    for c in legs:
        run(c)
        sizes[c] = file_bytes()
    for _ in range(3):
        for c in legs:
            t = time.perf_counter()
            st = run(c)
            legs[c].append((time.perf_counter() - t, st))
    out = {}
    for c, runs in legs.items():
        runs.sort(key=lambda x: x[0])
        secs = [x[0] for x in runs]
        ms, down = stats_of(runs[1][1])
        out[c + "_compressor"] = {"seconds": secs, "median_s": secs[1], "spread_s": secs[-1] - secs[0],
                                  "phases_s": runs[1][1]["phases"], "page_kernels_ms": ms, "bytes_downloaded": down,
                                  "file_bytes": sizes[c]}
        log("device pages, %s compressor: %s s, %d bytes down, %d bytes of files" % (
            c, ["%.2f" % x for x in secs], down, sizes[c]))
    h, d = out["host_compressor"], out["device_compressor"]
    out["device_over_host_compressor_seconds"] = d["median_s"] / h["median_s"]
    out["device_over_host_compressor_bytes_downloaded"] = d["bytes_downloaded"] / h["bytes_downloaded"]
    out["device_over_host_compressor_file_bytes"] = d["file_bytes"] / h["file_bytes"]
    out["device_compressor_faster_beyond_spread"] = h["median_s"] - d["median_s"] > max(h["spread_s"], d["spread_s"])
    return out


def bench_reads2ref_pages(a):
    """--reads2ref --parquet-encoder: `reads2ref` with the host's Parquet
    encoder (Arrow's writer over downloaded columns: unchanged code, the
    yardstick) and with -parquet_encoder device, in this process on the same
    file; per codec (snappy, gzip) each leg runs once after a warm-up of its
    own.  Per leg: wall seconds, the job's phases, the part files' bytes in
    all and per column (from the footers); the device leg also the page
    kernels' device-event times and the bytes it downloaded; and a third
    leg: the device encoder runs with readStart / readEnd as the per-read
    dictionary and as PLAIN int64 (reads2ref.READ_SPANS names the form kept
    per codec; the ratios are the kept form's).  Then "device_snappy": the
    device encoder under snappy with -parquet_compressor host next to device
    (_device_snappy_legs); --device-snappy-only runs nothing else."""
    import pyarrow.parquet as pq
    import torch
    from adam_amd import reads2ref as R
    t0 = time.perf_counter()
    sam = synthetic_sam(a.reads, a.len)
    log("generated %d bytes of SAM in %.1f s" % (len(sam), time.perf_counter() - t0))
    torch.zeros(1, device="cuda")
    work = a.dir or tempfile.mkdtemp(prefix="bench_reads2ref_pages_")
    os.makedirs(work, exist_ok=True)
    part_reads = a.part_reads if a.part_reads != 1 << 19 else R.DEFAULT_PART_READS
    res = {"metric": "adam reads2ref SAM -> ADAMPileup Parquet, -parquet_encoder host next to device: wall seconds of "
                     "one run after a warm-up, same process, same file",
           "reads": a.reads, "read_len": a.len, "input_bytes": len(sam), "part_reads": part_reads, "codecs": {}}
    try:
        src = os.path.join(work, "in.sam")
        with open(src, "wb") as fh:
            fh.write(sam)
        del sam

        kept_forms = dict(R.READ_SPANS)

        def leg(codec, encoder, spans="dictionary"):
            R.READ_SPANS = dict.fromkeys(R.READ_SPANS, spans)  # (the device leg's form of readStart / readEnd)
            out = os.path.join(work, "out_%s.adam" % encoder)
            run = lambda: R._reads2ref(src, out, codec, part_reads, a.partition_bytes, True, 0,  # noqa: E731
                                       parquet_encoder=encoder)
            run()
            t = time.perf_counter()
            st = run()
            dt = time.perf_counter() - t
            parts = sorted(f for f in os.listdir(out) if f.startswith("part-r-"))
            per_col = {}
            for f in parts:
                md = pq.ParquetFile(os.path.join(out, f)).metadata
                for g in range(md.num_row_groups):  # (Arrow's writer cuts a part into row groups of 1M rows)
                    rg = md.row_group(g)
                    for i in range(rg.num_columns):
                        c = rg.column(i)
                        per_col[c.path_in_schema] = per_col.get(c.path_in_schema, 0) + c.total_compressed_size
            r = {"seconds": dt, "rows": st["pileups"], "parts": st["parts"], "phases_s": st["phases"],
                 "file_bytes": sum(os.path.getsize(os.path.join(out, f)) for f in parts),
                 "column_bytes": per_col}
            if encoder == "device":
                r["page_kernels_ms"] = st["page_kernels_ms"]
                r["bytes_downloaded"] = st["page_bytes_downloaded"]
            else:  # the columns of every row and the four bitmaps
                rows = st["pileups"]
                r["bytes_downloaded"] = rows * (3 * 8 + 7 * 4 + 2) + 4 * ((rows + 63) // 64) * 8
            log("%s %s: %.2f s, %d bytes" % (codec, encoder, dt, r["file_bytes"]))
            shutil.rmtree(out, ignore_errors=True)
            return r

        def snappy_run(compressor):
            R.READ_SPANS = dict(kept_forms)
            return R._reads2ref(src, os.path.join(work, "out_snappy.adam"), "snappy", part_reads, a.partition_bytes,
                                True, 0, parquet_encoder="device", parquet_compressor=compressor)

        def snappy_bytes():
            out = os.path.join(work, "out_snappy.adam")
            return sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out) if f.startswith("part-r-"))

        for codec in () if a.device_snappy_only else ("snappy", "gzip"):
            kept = kept_forms[codec]
            h, d, p = leg(codec, "host"), leg(codec, "device", "dictionary"), leg(codec, "device", "plain")
            k = d if kept == "dictionary" else p
            res["codecs"][codec] = {"host": h, "device_dictionary_read_spans": d, "device_plain_read_spans": p,
                                    "read_spans_kept": kept,
                                    "device_over_host_seconds": k["seconds"] / h["seconds"],
                                    "device_over_host_file_bytes": k["file_bytes"] / h["file_bytes"]}
        res["device_snappy"] = _device_snappy_legs(
            snappy_run, snappy_bytes, lambda st: (st["page_kernels_ms"], st["page_bytes_downloaded"]))
    finally:
        R.READ_SPANS = kept_forms
        if not a.dir:
            shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(res))


def bench_transform_pages(a):
    """--parquet-encoder (without --reads2ref): `transform` to ADAM Parquet
    with the host's Parquet encoder (pyarrow over downloaded columns: unchanged
    code, the yardstick) and with -parquet_encoder device, in this process on
    the same reads: SAM and BAM input, gzip and snappy.  Each leg is warmed
    once and timed three times.  Per leg: the three wall times, their median
    and spread, the emit and close phases of the median run, the part files'
    bytes in all and per column (from the footers), the bytes downloaded; the
    device leg also the page kernels' device-event times.  Then
    "device_snappy" (SAM input): the device encoder under snappy with
    -parquet_compressor host next to device (_device_snappy_legs);
    --device-snappy-only runs nothing else and makes no BAM."""
    import pyarrow.compute as pc
    import pyarrow.parquet as pq
    import torch
    from adam_amd import adam_save, bqsr
    from adam_amd import transform as T
    from adam_amd.bam_writer import sam_to_bam_parallel
    t0 = time.perf_counter()
    sam = synthetic_sam(a.reads, a.len)
    log("generated %d bytes of SAM in %.1f s" % (len(sam), time.perf_counter() - t0))
    bam = b"" if a.device_snappy_only else sam_to_bam_parallel(  # (forks: before the GPU is touched)
        sam, min(16, len(os.sched_getaffinity(0))),
        progress=lambda i, n: log("bam slice %d / %d" % (i, n)) if i % 8 == 0 else None)
    torch.zeros(1, device="cuda")
    bqsr.Context.get(0).tune(bgzf=a.bgzf)
    work = a.dir or tempfile.mkdtemp(prefix="bench_transform_pages_")
    os.makedirs(work, exist_ok=True)
    res = {"metric": "transform SAM / BAM -> ADAM Parquet, -parquet_encoder host next to device: wall seconds of three "
                     "runs after a warm-up, same process, same reads",
           "reads": a.reads, "read_len": a.len, "part_reads": a.part_reads, "markdup": not a.no_markdup,
           "recalibrate": True, "legs": {}}
    try:
        src = {"sam": os.path.join(work, "in.sam"), "bam": os.path.join(work, "in.bam")}
        with open(src["sam"], "wb") as fh:
            fh.write(sam)
        with open(src["bam"], "wb") as fh:
            fh.write(bam)
        res["input_bytes"] = {k: os.path.getsize(v) for k, v in src.items()}
        del sam, bam

        def leg(kind, codec, encoder):
            out = os.path.join(work, "out_%s.adam" % encoder)
            run = lambda: T.transform(src[kind], out, mark_duplicates=not a.no_markdup, recalibrate=True,  # noqa: E731
                                      partition_bytes=a.partition_bytes, compression=codec, part_reads=a.part_reads,
                                      overwrite=True, parquet_encoder=encoder)
            run()
            runs = []
            for _ in range(3):
                t = time.perf_counter()
                st = run()
                runs.append((time.perf_counter() - t, st))
            runs.sort(key=lambda x: x[0])
            secs = [x[0] for x in runs]
            dt, st = runs[1]
            if st["reads"] != a.reads:
                raise SystemExit("transformed %d reads, expected %d" % (st["reads"], a.reads))
            parts = sorted(f for f in os.listdir(out) if f.startswith("part-r-"))
            per_col, raw_strings = {}, 0
            for f in parts:
                md = pq.ParquetFile(os.path.join(out, f)).metadata
                for g in range(md.num_row_groups):
                    rg = md.row_group(g)
                    for i in range(rg.num_columns):
                        c = rg.column(i)
                        per_col[c.path_in_schema] = per_col.get(c.path_in_schema, 0) + c.total_compressed_size
            r = {"seconds": secs, "median_s": dt, "spread_s": secs[-1] - secs[0], "parts": st["parts"],
                 "phases_s": st["phases"], "emit_s": st["phases"].get("emit"), "close_s": st["phases"].get("close"),
                 "file_bytes": sum(os.path.getsize(os.path.join(out, f)) for f in parts), "column_bytes": per_col}
            if encoder == "device":
                r["page_kernels_ms"] = st["pages"]["kernel_ms"]
                r["bytes_downloaded"] = st["pages"]["bytes_downloaded"]
            else:  # every column of every row: offsets, the strings' bytes, values and 23 bitmaps
                for f in parts:
                    t = pq.read_table(os.path.join(out, f), columns=list(adam_save.STR_COLS))
                    raw_strings += sum(pc.sum(pc.binary_length(c)).as_py() or 0 for c in t.columns)
                n, w = a.reads, (a.reads // 64 + 1) * 8
                r["bytes_downloaded"] = 6 * 4 * (n + st["parts"]) + raw_strings + 4 * 4 * n + 2 * 8 * n + 23 * w
            log("%s %s %s: %s s, %d bytes" % (kind, codec, encoder, ["%.2f" % x for x in secs], r["file_bytes"]))
            shutil.rmtree(out, ignore_errors=True)
            return r

        def snappy_run(compressor):
            st = T.transform(src["sam"], os.path.join(work, "out_snappy.adam"), mark_duplicates=not a.no_markdup,
                             recalibrate=True, partition_bytes=a.partition_bytes, compression="snappy",
                             part_reads=a.part_reads, overwrite=True, parquet_encoder="device",
                             parquet_compressor=compressor)
            if st["reads"] != a.reads:
                raise SystemExit("transformed %d reads, expected %d" % (st["reads"], a.reads))
            return st

        def snappy_bytes():
            out = os.path.join(work, "out_snappy.adam")
            return sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out) if f.startswith("part-r-"))

        for kind in () if a.device_snappy_only else ("sam", "bam"):
            for codec in ("gzip", "snappy"):
                h, d = leg(kind, codec, "host"), leg(kind, codec, "device")
                res["legs"]["%s_%s" % (kind, codec)] = {
                    "host": h, "device": d, "device_over_host_seconds": d["median_s"] / h["median_s"],
                    "device_over_host_file_bytes": d["file_bytes"] / h["file_bytes"],
                    "cigar_bytes_host_dictionary": h["column_bytes"].get("cigar"),
                    "cigar_bytes_device_plain": d["column_bytes"].get("cigar")}
        res["device_snappy"] = _device_snappy_legs(
            snappy_run, snappy_bytes, lambda st: (st["pages"]["kernel_ms"], st["pages"]["bytes_downloaded"]))
    finally:
        if not a.dir:
            shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(res))


def _thin_to_one_reference(sam: bytes):
    """(text, kept): the sorted SAM text without the reads LocusPredicate would
    keep that overlap the read kept before them.  The generator draws every
    read's bases and MD on its own, so two reads over one position disagree on
    the reference base there -- which `adam mpileup` refuses
    (REFERENCE_CONFLICT), as the reference asserts."""
    import re
    el = re.compile(rb"([0-9]+)([MIDNSHP=X])")
    out, kept, last_ref, last_end = [], 0, None, -1
    for line in sam.split(b"\n"):
        if not line:
            continue
        if line.startswith(b"@"):
            out.append(line)
            continue
        f = line.split(b"\t", 6)
        flag = int(f[1])
        if flag == 0 or flag & (0x4 | 0x100 | 0x200 | 0x400):  # LocusPredicate drops it anyway
            out.append(line)
            continue
        start = int(f[3]) - 1
        end = start + sum(int(n) for n, op in el.findall(f[5]) if op in b"MDN=X")
        if f[2] == last_ref and start < last_end:
            continue
        last_ref, last_end = f[2], end
        kept += 1
        out.append(line)
    return b"\n".join(out) + b"\n", kept


def bench_mpileup(a):
    """the --mpileup measurements (see the module doc)"""
    import torch
    from adam_amd import mpileup as M
    from adam_amd import reads2ref as R
    from adam_amd.transform import transform
    t0 = time.perf_counter()
    sam = synthetic_sam(a.reads, a.len)
    log("generated %d bytes of SAM in %.1f s" % (len(sam), time.perf_counter() - t0))
    torch.zeros(1, device="cuda")
    work = a.dir or tempfile.mkdtemp(prefix="bench_mpileup_")
    os.makedirs(work, exist_ok=True)
    raw, srt, src, small = (os.path.join(work, n) for n in ("raw.sam", "sorted.sam", "in.sam", "small.sam"))
    part_reads = a.part_reads if a.part_reads != 1 << 19 else R.DEFAULT_PART_READS

    def timed(f):
        t = time.perf_counter()
        st = f()
        return time.perf_counter() - t, st

    try:
        with open(raw, "wb") as fh:
            fh.write(sam)
        del sam
        s_sort, _ = timed(lambda: transform(raw, srt, sort_reads=True, partition_bytes=a.partition_bytes,
                                            overwrite=True))
        with open(srt, "rb") as fh:
            text, kept = _thin_to_one_reference(fh.read())
        n_lines = text.count(b"\n") - sum(1 for l in text.split(b"\n", 64)[:64] if l.startswith(b"@"))
        log("sorted in %.1f s; %d reads left, %d of them kept by LocusPredicate" % (s_sort, n_lines, kept))
        with open(src, "wb") as fh:
            fh.write(text)
        n_small = min(n_lines, a.restatement_reads)
        cut = 0
        while text[cut:cut + 1] == b"@":
            cut = text.index(b"\n", cut) + 1
        for _ in range(n_small):
            cut = text.index(b"\n", cut) + 1
        small_text = text[:cut]
        with open(small, "wb") as fh:
            fh.write(small_text)
        del text
        out_m, out_r, out_s = (os.path.join(work, n) for n in ("mpileup.txt", "r2r.adam", "small.txt"))
        mp = lambda i=src, o=out_m: M.mpileup(i, o)
        r2r = lambda: R._reads2ref(src, out_r, a.compression, part_reads, a.partition_bytes, True, 0)
        log("warm-up runs")
        mp()
        r2r()
        log("timed runs")
        s_m, st_m = timed(mp)
        s_r, st_r = timed(r2r)
        size = lambda d: sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
        res = {"metric": "adam mpileup SAM -> pileup text next to adam reads2ref on the same reads, one run each after "
                         "a warm-up in one process: end-to-end seconds and phase split (host clock), mpileup's stages "
                         "by device events",
               "input": "%d synthetic reads of %d bases, transform -sort_reads, then without the LocusPredicate-kept "
                        "reads that overlap the kept read before them (the generator's reads do not share a "
                        "reference: overlapping ones are a REFERENCE_CONFLICT)" % (a.reads, a.len),
               "reads": n_lines, "read_len": a.len, "input_bytes": os.path.getsize(src),
               "mpileup": {"seconds": s_m, "kept_reads": st_m["kept"], "events": st_m["events"],
                           "lines": st_m["lines"], "text_bytes": st_m["bytes"], "phases_s": st_m["phases"],
                           "kernels_ms": st_m["kernel_ms"], "window_bytes": M.DEFAULT_WINDOW_BYTES,
                           "events_per_s": st_m["events"] / s_m if s_m else None},
               "reads2ref": {"seconds": s_r, "rows": st_r["pileups"], "output_bytes": size(out_r),
                             "compression": a.compression, "phases_s": st_r["phases"]},
               "mpileup_over_reads2ref": s_m / s_r}
        # the restatement, single-threaded, on the first reads; the command on the same reads must agree
        if n_small:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            from _adam_ref import convert_sam
            from _mpileup_ref import mpileup as restated
            s_p, want = timed(lambda: restated(convert_sam(small_text)).encode("latin-1"))
            s_s, _ = timed(lambda: mp(small, out_s))
            with open(out_s, "rb") as fh:
                assert fh.read() == want, "the command and the restatement differ"
            res["python_restatement"] = {"reads": n_small, "seconds": s_p, "text_bytes": len(want),
                                         "mpileup_seconds_same_reads": s_s}
        log("mpileup %.2f s (%d events, %d lines), reads2ref %.2f s (%d rows), kernels %s"
            % (s_m, st_m["events"], st_m["lines"], s_r, st_r["pileups"], st_m["kernel_ms"]))
    finally:
        if not a.dir:
            shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(res))


def bench_realign_targets(a):
    """the --realign-targets measurements (see the module doc)"""
    import ctypes

    import numpy as np
    import torch
    from adam_amd import _capi
    from adam_amd import mpileup as M
    from adam_amd import reads2ref as R
    from adam_amd import realignment_targets as RT
    from adam_amd.sam import SamText
    t0 = time.perf_counter()
    sam = synthetic_sam(a.reads, a.len)
    log("generated %d bytes of SAM in %.1f s" % (len(sam), time.perf_counter() - t0))
    torch.zeros(1, device="cuda")
    work = a.dir or tempfile.mkdtemp(prefix="bench_realign_targets_")
    os.makedirs(work, exist_ok=True)
    src, small = os.path.join(work, "in.sam"), os.path.join(work, "small.sam")

    def timed(f):
        t = time.perf_counter()
        st = f()
        return time.perf_counter() - t, st

    def targets(path):
        st = {}
        out = RT.realignment_targets(path, stats=st)
        return st, out

    try:
        with open(src, "wb") as fh:
            fh.write(sam)
        n_small = min(a.reads, a.restatement_reads)
        cut = 0
        while sam[cut:cut + 1] == b"@":
            cut = sam.index(b"\n", cut) + 1
        for _ in range(n_small):
            cut = sam.index(b"\n", cut) + 1
        small_text = sam[:cut]
        with open(small, "wb") as fh:
            fh.write(small_text)
        log("warm-up run")
        targets(src)
        log("timed run")
        s_t, (st, out) = timed(lambda: targets(src))
        ts, te = out["target_start"], out["target_end"]
        n_ind = np.diff(out["indel_offset"])
        res = {"metric": "indel realignment targets (RealignmentTargetFinder) of SAM text, one run after a warm-up in "
                         "one process: end-to-end seconds and phase split (host clock), the stages by device events "
                         "(fold_host: the serial fold, host clock)",
               "input": "%d synthetic reads of %d bases as generated, unsorted, every read taken" % (a.reads, a.len),
               "reads": st["reads"], "read_len": a.len, "input_bytes": os.path.getsize(src),
               "realign_targets": {"seconds": s_t, "rows": st["rows"], "candidates": st["candidates"],
                                   "targets": st["targets"], "indel_ranges": st["indels"], "snp_ranges": st["snps"],
                                   "phases_s": st["phases"], "kernels_ms": st["kernel_ms"],
                                   "rows_per_s": st["rows"] / s_t if s_t else None,
                                   "targets_with_indels": int((n_ind > 0).sum()),
                                   "longest_target": int((te - ts + 1).max()) if len(ts) else 0,
                                   "candidates_per_target": st["candidates"] / st["targets"] if st["targets"] else None}}
        # the pileup walk alone (reads2ref's prepare over all reads) and mpileup, on the same file
        with open(src, "rb") as fh:
            data = fh.read()
        s = SamText(data)
        try:
            L = R._lib()
            sz = R.PileupSizes()
            prep = lambda: _capi.check(L.bqsr_sam_pileup_prepare(s.ctx.handle, s.h, 0, s.counts().n_reads, None,
                                                                 ctypes.byref(sz)))
            prep()
            s_p, _ = timed(prep)
            res["reads2ref_prepare"] = {"seconds": s_p, "rows": sz.n_rows, "count_kernel_ms": R.kernel_times()[0]}
        finally:
            s.close()
        del data
        try:
            s_m, st_m = timed(lambda: M.mpileup(src, os.path.join(work, "mpileup.txt")))
            res["mpileup"] = {"seconds": s_m, "events": st_m["events"], "lines": st_m["lines"]}
        except _capi.BQSRError as e:
            res["mpileup"] = {"refused": e.name, "message": str(e)[:200]}
        if n_small:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            from _adam_ref import convert_sam
            import _realign_targets_ref as ref
            s_r, want = timed(lambda: ref.as_arrays(ref.find_targets(convert_sam(small_text))))
            s_s, (st_s, got) = timed(lambda: targets(small))
            assert all(np.array_equal(got[k], want[k]) for k in RT.COLUMNS), "the device and the restatement differ"
            res["python_restatement"] = {"reads": n_small, "seconds": s_r, "targets": st_s["targets"],
                                         "realign_targets_seconds_same_reads": s_s}
        log("realign targets %.2f s (%d rows, %d candidates, %d targets), kernels %s"
            % (s_t, st["rows"], st["candidates"], st["targets"], st["kernel_ms"]))
    finally:
        if not a.dir:
            shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(res))


def bench_aggregate(a):
    """the --aggregate measurements (see the module doc)"""
    import torch
    from adam_amd import aggregate_pileups as AP
    from adam_amd import reads2ref as R
    t0 = time.perf_counter()
    sam = synthetic_sam(a.reads, a.len)
    log("generated %d bytes of SAM in %.1f s" % (len(sam), time.perf_counter() - t0))
    torch.zeros(1, device="cuda")
    work = a.dir or tempfile.mkdtemp(prefix="bench_aggregate_")
    os.makedirs(work, exist_ok=True)
    src, small = os.path.join(work, "in.sam"), os.path.join(work, "small.sam")
    part_reads = a.part_reads if a.part_reads != 1 << 19 else R.DEFAULT_PART_READS

    def timed(f):
        t = time.perf_counter()
        st = f()
        return time.perf_counter() - t, st

    try:
        with open(src, "wb") as fh:
            fh.write(sam)
        n_small = min(a.reads, a.restatement_reads)
        cut = 0
        while sam[cut:cut + 1] == b"@":
            cut = sam.index(b"\n", cut) + 1
        for _ in range(n_small):
            cut = sam.index(b"\n", cut) + 1
        with open(small, "wb") as fh:
            fh.write(sam[:cut])
        del sam
        out_r, out_a, out_s = (os.path.join(work, n) for n in ("r2r.adam", "agg.adam", "small.adam"))
        r2r = lambda: R._reads2ref(src, out_r, a.compression, part_reads, a.partition_bytes, True, 0)
        agg = lambda o=out_a, i=src: AP.aggregate_pileups(i, o, a.compression, partition_bytes=a.partition_bytes,
                                                          overwrite=True, part_reads=part_reads)
        log("warm-up runs")
        r2r()
        agg()
        log("timed runs")
        s_r, st_r = timed(r2r)
        s_a, st_a = timed(agg)
        size = lambda d: sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
        res = {"metric": "adam aggregate_pileups SAM -> aggregated ADAMPileup Parquet next to adam reads2ref on the "
                         "same reads: end-to-end seconds and phase split (host clock), the aggregation's stages by "
                         "device events",
               "reads": a.reads, "read_len": a.len, "compression": a.compression, "part_reads": part_reads,
               "reads2ref": {"seconds": s_r, "rows": st_r["pileups"], "output_bytes": size(out_r),
                             "phases_s": st_r["phases"]},
               "aggregate_pileups": {"seconds": s_a, "rows_in": st_a["rows_in"], "rows_out": st_a["rows_out"],
                                     "output_bytes": size(out_a), "phases_s": st_a["phases"],
                                     "kernels_ms": st_a["kernel_ms"], "parts": st_a["parts"]},
               "aggregate_over_reads2ref": s_a / s_r}
        # the restatement, single-threaded, on the first reads; the command on the same reads must agree
        if n_small:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import glob
            import pyarrow as pa
            import pyarrow.parquet as pq
            from _adam_ref import convert_sam
            from _pileup_agg_ref import aggregate
            from _pileup_gen import assert_rows, run_date
            from _pileup_ref import reads_to_pileups
            with open(small, "rb") as fh:
                text = fh.read()
            s_p, want = timed(lambda: aggregate(reads_to_pileups(convert_sam(text, run_date))))
            s_s, _ = timed(lambda: agg(out_s, small))
            got = pa.concat_tables([pq.read_table(f) for f in sorted(glob.glob(os.path.join(out_s, "part-r-*.parquet")))])
            assert_rows(got, want)
            res["python_restatement"] = {"reads": n_small, "seconds": s_p, "rows_out": len(want),
                                         "aggregate_pileups_seconds_same_reads": s_s}
        log("reads2ref %.2f s (%d rows), aggregate_pileups %.2f s (%d -> %d rows), kernels %s"
            % (s_r, st_r["pileups"], s_a, st_a["rows_in"], st_a["rows_out"], st_a["kernel_ms"]))
    finally:
        if not a.dir:
            shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(res))


def bench_bam_out(a):
    t0 = time.perf_counter()
    data = synthetic_sam(a.reads, a.len, p_q2tail=0.0)
    log("generated %d bytes in %.1f s" % (len(data), time.perf_counter() - t0))
    import torch
    from adam_amd import _capi
    from adam_amd import transform as T
    torch.zeros(1, device="cuda")
    work = a.dir or tempfile.mkdtemp(prefix="bench_adam_")
    os.makedirs(work, exist_ok=True)
    src = os.path.join(work, "in.sam")
    with open(src, "wb") as fh:
        fh.write(data)
    n_bytes = len(data)
    del data

    def leg(out, recal, **kw):
        best, times = None, []
        for i in range(1 + max(1, a.reps)):  # the first run warms
            log("%s transform -> %s %s" % ("warm-up" if i == 0 else "timed", os.path.basename(out), kw or ""))
            t = time.perf_counter()
            st = T.transform(src, out, mark_duplicates=not a.no_markdup, recalibrate=recal,
                             partition_bytes=a.partition_bytes, overwrite=True, **kw)
            dt = time.perf_counter() - t
            if i:
                times.append(dt)
                if best is None or dt < best[0]:
                    best = (dt, st)
        if best[1]["reads"] != a.reads:
            raise SystemExit("transformed %d reads, expected %d" % (best[1]["reads"], a.reads))
        return best[0], best[1], times

    peak = 8e12

    def bam_result(dt, st, times, path, what):
        b = st["bam"]
        k1 = b["text_bytes"] / (b["len_ms"] * 1e-3) if b["len_ms"] else None
        moved2 = b["text_bytes"] + b["record_bytes"]
        k2 = moved2 / (b["write_ms"] * 1e-3) if b["write_ms"] else None
        ph = st.get("phases") or {}
        r = {"seconds": dt, "seconds_all": times, "seconds_spread": max(times) - min(times),
             "reads_per_s": a.reads / dt, "output_bytes": os.path.getsize(path), "compressor": what,
             "phases_s": ph, "emit_s": ph.get("emit"), "close_s": ph.get("close"),
             "record_bytes": b["record_bytes"], "downloaded_bytes": b["downloaded_bytes"],
             "compress_s": b["compress_s"],
             "compress_MB_per_s": b["record_bytes"] / b["compress_s"] / 1e6 if b["compress_s"] else None,
             "kernels": {"len_ms": b["len_ms"], "len_bytes_read": b["text_bytes"], "len_bytes_per_s": k1,
                         "len_share_of_8TBps": k1 / peak if k1 else None,
                         "write_ms": b["write_ms"], "write_bytes_moved": moved2, "write_bytes_per_s": k2,
                         "write_share_of_8TBps": k2 / peak if k2 else None}}
        if b["compressor"] == "device":
            ms = b["deflate_ms"] + b["pack_ms"]
            r["kernels"].update({"deflate_ms": b["deflate_ms"], "pack_ms": b["pack_ms"],
                                 "deflate_GB_per_s_of_stream": b["record_bytes"] / (ms * 1e-3) / 1e9 if ms else None})
        return r

    try:
        recal, refused = True, None
        out_bam = os.path.join(work, "out.bam")
        try:
            bdt, bst, bts = leg(out_bam, True, bam_level=a.bam_level)
        except _capi.BQSRError as e:
            if e.status != _capi.UNSUPPORTED:
                raise
            recal, refused = False, str(e)
            log("BAM refused the recalibrated records (%s): every leg without BQSR" % e)
            bdt, bst, bts = leg(out_bam, False, bam_level=a.bam_level)
        bam = bam_result(bdt, bst, bts, out_bam, "host threads, level %d" % a.bam_level)
        bam["level"] = a.bam_level
        sdt, sst, sts = leg(os.path.join(work, "out.sam"), recal)
        sam_bytes = os.path.getsize(os.path.join(work, "out.sam"))
        # the host compressor at level 1 and the device compressor: the same run, the same input
        l1 = bam_result(*leg(out_bam, recal, bam_level=1), out_bam, "host threads, level 1")
        l1["level"] = 1
        dev = bam_result(*leg(out_bam, recal, bam_compressor="device"), out_bam, "device")
    finally:
        if not a.dir:
            shutil.rmtree(work, ignore_errors=True)
    print(json.dumps({
        "metric": "transform SAM -> BAM (records encoded on the device; BGZF members by host threads at two levels "
                  "and by the device) next to SAM -> SAM text, same input, same run; %sMarkDuplicates%s" % (
                      "" if not a.no_markdup else "no ", ", BQSR" if recal else ", no BQSR"),
        "reads": a.reads, "read_len": a.len, "input_bytes": n_bytes, "recalibrate": recal, "refused": refused,
        "reps": max(1, a.reps),
        "bam": bam, "bam_level1": l1, "bam_device": dev,
        "sam": {"seconds": sdt, "seconds_all": sts, "seconds_spread": max(sts) - min(sts),
                "reads_per_s": a.reads / sdt, "output_bytes": sam_bytes, "phases_s": sst.get("phases")}}))


def sorted_by_position(data: bytes) -> bytes:
    """a SAM text's records in (@SQ index, POS) order, reads without an RNAME last, ties in input order"""
    head, recs = [], []
    for l in data.split(b"\n"):
        if l.startswith(b"@"):
            head.append(l)
        elif l:
            recs.append(l)
    ref = {l.split(b"\t")[1][3:]: i for i, l in enumerate(h for h in head if h.startswith(b"@SQ"))}

    def key(l):
        f = l.split(b"\t", 4)
        return (ref[f[2]], int(f[3])) if f[2] in ref else (len(ref), 0)
    recs.sort(key=key)
    return b"\n".join(head + recs) + b"\n"


def bench_bam_index(a):
    """--bam-out --bam-index: see the module doc"""
    import inspect
    t0 = time.perf_counter()
    data = sorted_by_position(synthetic_sam(a.reads, a.len, p_q2tail=0.0))
    log("generated and sorted %d bytes in %.1f s" % (len(data), time.perf_counter() - t0))
    import torch
    from adam_amd import transform as T
    torch.zeros(1, device="cuda")
    has_index = "bam_index" in inspect.signature(T.transform).parameters
    work = a.dir or tempfile.mkdtemp(prefix="bench_adam_")
    os.makedirs(work, exist_ok=True)
    src, out = os.path.join(work, "in.sam"), os.path.join(work, "out.bam")
    with open(src, "wb") as fh:
        fh.write(data)
    n_bytes = len(data)
    del data
    reps = max(3, a.reps)

    def leg(**kw):
        runs = []
        for i in range(1 + reps):  # the first run warms
            log("%s transform -> out.bam %s" % ("warm-up" if i == 0 else "timed", kw))
            t = time.perf_counter()
            st = T.transform(src, out, mark_duplicates=not a.no_markdup, partition_bytes=a.partition_bytes,
                             overwrite=True, **kw)
            runs.append((time.perf_counter() - t, st))
        if runs[-1][1]["reads"] != a.reads:
            raise SystemExit("transformed %d reads, expected %d" % (runs[-1][1]["reads"], a.reads))
        times = [dt for dt, _ in runs[1:]]
        dt, st = min(runs[1:], key=lambda r: r[0])
        b = st["bam"]
        r = {"seconds": dt, "seconds_all": times, "seconds_spread": max(times) - min(times),
             "reads_per_s": a.reads / dt, "output_bytes": os.path.getsize(out), "emit_s": st["phases"].get("emit"),
             "close_s": st["phases"].get("close")}
        if kw.get("bam_index"):
            r.update({"index_bytes": b["index_bytes"], "index_chunks": b["index_chunks"], "index_bins": b["index_bins"],
                      "index_device_bytes": b["index_device_bytes"], "index_stage_ms": b["index_ms"],
                      "index_device_ms": sum(v for k, v in b["index_ms"].items() if not k.endswith("_host")),
                      "member_walk_host_s": b["index_walk_s"],
                      "serialize_host_ms": b["index_ms"]["serialize_host"]})
        return r

    res = {}
    restated = None
    try:
        for name, kw in (("host", {"bam_level": a.bam_level}), ("device", {"bam_compressor": "device"})):
            res[name] = {"no_index": leg(**kw)}
            if not has_index:
                continue
            res[name]["index"] = leg(bam_index=True, **kw)
            res[name]["index_minus_no_index_s"] = res[name]["index"]["seconds"] - res[name]["no_index"]["seconds"]
            if name == "host":  # the external pass the flag replaces, on the finished file; and the same bytes
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                import _bai_ref
                with open(out, "rb") as fh:
                    bam = fh.read()
                with open(out + ".bai", "rb") as fh:
                    bai = fh.read()
                t = time.perf_counter()
                want = _bai_ref.bai_of_bam(bam)
                restated = {"seconds": time.perf_counter() - t, "equal": want == bai,
                            "what": "tests/_bai_ref.bai_of_bam on the finished file: inflate, walk every record, build "
                                    "the index serially (single-threaded Python)"}
                del bam
                if not restated["equal"]:
                    raise SystemExit("the device's index differs from the restatement's")
    finally:
        if not a.dir:
            shutil.rmtree(work, ignore_errors=True)
    print(json.dumps({
        "metric": "transform SAM -> BAM with and without -bam_index (the .bai built on the device), reads sorted by "
                  "position, same input, same process; %sMarkDuplicates, no BQSR" % ("" if not a.no_markdup else "no "),
        "reads": a.reads, "read_len": a.len, "input_bytes": n_bytes, "reps": reps, "bam_level": a.bam_level,
        "index_legs": has_index,
        "legs": res, "restatement": restated,
        "not_measured": "real coverage (the synthetic reads spread evenly), inputs above one partition"}))


def bench_bam_region(a):
    """--bam-region: see the module doc"""
    import statistics
    t0 = time.perf_counter()
    data = sorted_by_position(synthetic_sam(a.reads, a.len, p_q2tail=0.0))
    log("generated and sorted %d bytes in %.1f s" % (len(data), time.perf_counter() - t0))
    # a region holding about 1 % of the reads: around the middle of the reference with the most reads
    recs = [l.split(b"\t", 4) for l in data.split(b"\n") if l and not l.startswith(b"@")]
    placed = [(f[2], int(f[3])) for f in recs if f[2] != b"*"]
    name = placed[len(placed) // 2][0]
    pos = [q for n, q in placed if n == name]
    k = max(1, a.reads // 200)
    mid = len(pos) // 2
    region = "%s:%d-%d" % (name.decode(), pos[max(0, mid - k)], pos[min(len(pos) - 1, mid + k)])
    del recs, placed, pos
    import torch
    from adam_amd import bam_index as BI
    from adam_amd import flagstat as F
    from adam_amd import transform as T
    torch.zeros(1, device="cuda")
    work = a.dir or tempfile.mkdtemp(prefix="bench_adam_")
    os.makedirs(work, exist_ok=True)
    src, bam = os.path.join(work, "in.sam"), os.path.join(work, "out.bam")
    with open(src, "wb") as fh:
        fh.write(data)
    n_bytes = len(data)
    del data
    reps = max(3, a.reps)
    pb = a.partition_bytes

    def summary(times):
        return {"seconds_median": statistics.median(times), "seconds_all": times,
                "seconds_spread": max(times) - min(times)}

    try:
        # the BAM and, beside it, the index transform builds while it writes: its stages, for the same reads
        written = []
        for i in range(1 + reps):
            log("%s transform -> out.bam -bam_index" % ("warm-up" if i == 0 else "timed"))
            t = time.perf_counter()
            st = T.transform(src, bam, mark_duplicates=False, partition_bytes=pb, overwrite=True, bam_index=True)
            written.append((time.perf_counter() - t, st))
        with open(bam + ".bai", "rb") as fh:
            theirs = fh.read()
        legs = {"bam_index": [], "flagstat_whole": [], "flagstat_region": []}
        last = {}
        for i in range(1 + reps):  # the first round warms; the legs alternate
            for leg in legs:
                log("%s %s" % ("warm-up" if i == 0 else "timed", leg))
                t = time.perf_counter()
                if leg == "bam_index":
                    st = BI.bam_index(bam, out=os.path.join(work, "again.bai"), overwrite=True)
                elif leg == "flagstat_whole":
                    st = F._flagstat(bam, 0, pb)[2]
                else:
                    st = F._flagstat(bam, 0, pb, region)[2]
                if i:
                    legs[leg].append(time.perf_counter() - t)
                last[leg] = st
        with open(os.path.join(work, "again.bai"), "rb") as fh:
            equal = fh.read() == theirs
        if not equal:
            raise SystemExit("bam_index on the finished file differs from the index transform wrote")
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import _bai_ref
        with open(bam, "rb") as fh:
            raw = fh.read()
        t = time.perf_counter()
        restated = _bai_ref.bai_of_bam(raw) == theirs
        t_restated = time.perf_counter() - t
        del raw
        if not restated:
            raise SystemExit("the index differs from the restatement's")
        bi, fr, fw = last["bam_index"], last["flagstat_region"], last["flagstat_whole"]
        region_s, whole_s = summary(legs["flagstat_region"]), summary(legs["flagstat_whole"])
        gain = whole_s["seconds_median"] - region_s["seconds_median"]
        spread = max(region_s["seconds_spread"], whole_s["seconds_spread"])
        print(json.dumps({
            "metric": "bam_index on an existing BAM, and flagstat -region through the index, against the whole file; "
                      "reads sorted by position, all legs in one process, warmed, %d timed runs each, alternating" % reps,
            "reads": a.reads, "read_len": a.len, "input_bytes": n_bytes, "bam_bytes": os.path.getsize(bam),
            "reps": reps, "region": region,
            "bam_index": dict(summary(legs["bam_index"]), stage_ms=bi["index_ms"],
                              device_ms=sum(v for k, v in bi["index_ms"].items() if not k.endswith("_host")),
                              windows_device=bi["windows_device"], windows_host=bi["windows_host"],
                              members=bi["members_total"], index_bytes=bi["index_bytes"], equal_to_transform_s=equal),
            "transform_bam_index": dict(summary([dt for dt, _ in written[1:]]),
                                        stage_ms=written[-1][1]["bam"]["index_ms"],
                                        member_walk_host_s=written[-1][1]["bam"]["index_walk_s"]),
            "restatement": {"seconds": t_restated, "equal": restated,
                            "what": "tests/_bai_ref.bai_of_bam on the same file (single-threaded Python)"},
            "flagstat_whole": dict(whole_s, reads=fw["reads"], phases=fw["phases"]),
            "flagstat_region": dict(region_s, reads=fr["reads"], phases=fr["phases"],
                                    members_read=fr.get("members_read"), members_total=fr.get("members_total"),
                                    records_seen=fr.get("records_seen"), records_kept=fr.get("records_kept"),
                                    filter_ms=fr.get("filter_ms"), share_of_reads=fr["reads"] / a.reads),
            "region_faster_by_s": gain, "region_faster_than_spread": gain > spread,
            "not_measured": "BAMs written by other tools, real coverage (the synthetic reads spread evenly), files "
                            "above one window"}))
    finally:
        if not a.dir:
            shutil.rmtree(work, ignore_errors=True)


def bench_adam2sam(a):
    """--adam2sam: the synthetic reads written once as .adam, then in one
    process, after a warm-up each, max(3, --reps) timed runs of ADAM -> SAM and
    ADAM -> BAM (adam2sam) next to SAM -> SAM and SAM -> BAM (transform without
    MarkDuplicates or BQSR: the same sinks over the same records).  Phases of
    the adam2sam legs: the Parquet read (Arrow's decode on host threads),
    the header synthesis, the chunk buffers and their upload, the two line
    kernels by device events, the parse, emit, close.  The same reads are
    also parsed as BAM input (bam_ingest.hip renders their lines with
    bam_lines_len / bam_lines_write): under rocprofv3 --kernel-trace --stats
    one run gives both pairs of kernels."""
    t0 = time.perf_counter()
    data = synthetic_sam(a.reads, a.len, p_q2tail=0.0)
    log("generated %d bytes in %.1f s" % (len(data), time.perf_counter() - t0))
    import torch
    from adam_amd import transform as T
    from adam_amd.adam2sam import adam2sam
    from adam_amd.sam import SamText
    torch.zeros(1, device="cuda")
    work = a.dir or tempfile.mkdtemp(prefix="bench_adam_")
    os.makedirs(work, exist_ok=True)
    src, adam, bam_in = (os.path.join(work, n) for n in ("in.sam", "in.adam", "in.bam"))
    with open(src, "wb") as fh:
        fh.write(data)
    n_bytes = len(data)
    header_bytes = len(T.sam_partitions(data, len(data))[0])
    del data
    reps = max(3, a.reps)

    def leg(run, out, **kw):
        runs = []
        for i in range(1 + reps):  # the first run warms
            log("%s %s -> %s %s" % ("warm-up" if i == 0 else "timed", run.__name__, os.path.basename(out), kw or ""))
            t = time.perf_counter()
            st = run(adam if run is adam2sam else src, out, overwrite=True, **kw)
            runs.append((time.perf_counter() - t, st))
        if runs[-1][1]["reads"] != a.reads:
            raise SystemExit("wrote %d reads, expected %d" % (runs[-1][1]["reads"], a.reads))
        times = [dt for dt, _ in runs[1:]]
        dt, st = min(runs[1:], key=lambda r: r[0])
        r = {"seconds": dt, "seconds_all": times, "seconds_spread": max(times) - min(times),
             "reads_per_s": a.reads / dt, "output_bytes": os.path.getsize(out), "phases_s": st.get("phases")}
        if "adam_lines" in st:
            L = st["adam_lines"]
            r["lines"] = dict(L, len_ms_all=[s["adam_lines"]["len_ms"] for _, s in runs[1:]],
                              write_ms_all=[s["adam_lines"]["write_ms"] for _, s in runs[1:]])
        return r

    res = {}
    try:
        t = time.perf_counter()
        T.transform(src, adam, compression=a.compression, part_reads=a.part_reads, overwrite=True)
        T.transform(src, bam_in, bam_level=1, overwrite=True)
        log("wrote in.adam and in.bam in %.1f s" % (time.perf_counter() - t))
        adam_bytes = sum(os.path.getsize(os.path.join(adam, f)) for f in os.listdir(adam))
        res["adam_to_sam"] = leg(adam2sam, os.path.join(work, "a.sam"))
        with open(os.path.join(work, "a.sam"), "rb") as fh:  # the record text the two kernels wrote
            head = fh.read(1 << 16)
        text_bytes = res["adam_to_sam"]["output_bytes"] - len(T.sam_partitions(head, len(head))[0])
        res["adam_to_bam"] = leg(adam2sam, os.path.join(work, "a.bam"), bam_level=a.bam_level)
        res["adam_to_bam_device"] = leg(adam2sam, os.path.join(work, "a.bam"), bam_compressor="device")
        res["sam_to_sam"] = leg(T.transform, os.path.join(work, "s.sam"))
        res["sam_to_bam"] = leg(T.transform, os.path.join(work, "s.bam"), bam_level=a.bam_level)
        res["sam_to_bam_device"] = leg(T.transform, os.path.join(work, "s.bam"), bam_compressor="device")
        ingest = []
        for i in range(1 + reps):  # BAM input: bam_lines_len / bam_lines_write over the same reads
            t = time.perf_counter()
            s = SamText.read(bam_in)
            n_text = s.counts().text_bytes
            s.close()
            ingest.append(time.perf_counter() - t)
        for k in ("adam_to_sam", "adam_to_bam", "adam_to_bam_device"):
            L = res[k]["lines"]
            body = L["record_text_bytes"] = text_bytes
            L["len_ns_per_text_byte"] = min(L["len_ms_all"]) * 1e6 / body
            L["write_ns_per_text_byte"] = min(L["write_ms_all"]) * 1e6 / body
            L["write_GB_per_s_of_text"] = body / (min(L["write_ms_all"]) * 1e-3) / 1e9
    finally:
        if not a.dir:
            shutil.rmtree(work, ignore_errors=True)
    print(json.dumps({
        "metric": "adam2sam: ADAM Parquet -> SAM / BAM (lines rendered on the device) next to transform SAM -> SAM / "
                  "BAM, same reads, same process, no MarkDuplicates, no BQSR",
        "reads": a.reads, "read_len": a.len, "sam_bytes": n_bytes, "sam_record_bytes": n_bytes - header_bytes,
        "adam_bytes": adam_bytes, "adam_compression": a.compression, "reps": reps, "bam_level": a.bam_level,
        "legs": res,
        "bam_input_parse": {"seconds_all": ingest[1:], "text_bytes": n_text,
                            "what": "SamText.read of the same reads as BAM (device inflate, bam_lines_len / "
                                    "bam_lines_write, the parse): the kernels' times come from a rocprofv3 "
                                    "--kernel-trace --stats run of this leg"},
        "not_measured": "real data (the synthetic reads carry two or three short tags), inputs beyond one resident "
                        "table"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--adam2sam", action="store_true",
                    help="measure adam2sam (ADAM -> SAM / BAM) next to transform SAM -> SAM / BAM instead")
    ap.add_argument("--bam-index", action="store_true",
                    help="--bam-out: measure -bam_index instead (legs with and without the index, both compressors)")
    ap.add_argument("--bam-region", action="store_true",
                    help="measure bam_index on an existing BAM and flagstat -region through its index")
    ap.add_argument("--bam-out", action="store_true",
                    help="measure transform SAM -> BAM next to SAM -> SAM text instead of the ADAM transform")
    ap.add_argument("--bam-level", type=int, default=6, help="--bam-out: the BGZF members' DEFLATE level")
    ap.add_argument("--reads2ref", action="store_true", help="measure adam reads2ref instead of the transform")
    ap.add_argument("--parquet-encoder", action="store_true",
                    help="measure -parquet_encoder device next to the host encoder, snappy and gzip: of the transform "
                         "(SAM and BAM input), or with --reads2ref of reads2ref")
    ap.add_argument("--device-snappy-only", action="store_true",
                    help="--parquet-encoder: only the device encoder's snappy legs, -parquet_compressor host next to "
                         "device")
    ap.add_argument("--aggregate", action="store_true",
                    help="measure adam aggregate_pileups next to adam reads2ref instead of the transform")
    ap.add_argument("--mpileup", action="store_true",
                    help="measure adam mpileup next to adam reads2ref instead of the transform")
    ap.add_argument("--realign-targets", action="store_true",
                    help="measure the indel realignment targets instead of the transform")
    ap.add_argument("--restatement-reads", type=int, default=200_000,
                    help="--aggregate: reads the Python restatement is timed on (0: skip it)")
    ap.add_argument("--flagstat", action="store_true", help="measure adam flagstat instead of the transform")
    ap.add_argument("--print-tags", action="store_true", help="measure adam print_tags instead of the transform")
    ap.add_argument("--variant-lib", default=None,
                    help="--print-tags: a library built with the other histogram form, for the A/B of the scan kernel")
    ap.add_argument("--scan-only", default=None, metavar="SAM", help=argparse.SUPPRESS)
    ap.add_argument("--kernel-reads", type=int, default=64_000_000,
                    help="--flagstat: random reads for the Arrow-form kernel alone")
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--len", type=int, default=100)
    ap.add_argument("--bam", action="store_true")
    ap.add_argument("--bgzf", type=int, default=1, help="BAM: 1 inflate on the device (default), 0 on host threads")
    ap.add_argument("--no-markdup", action="store_true")
    ap.add_argument("--sort_reads", action="store_true", help="transform -sort_reads")
    ap.add_argument("--compression", default="snappy")
    ap.add_argument("--part-reads", type=int, default=1 << 19)
    ap.add_argument("--partition-bytes", type=int, default=8 << 30)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--dir", default=None, help="scratch directory (default: a temporary one)")
    a = ap.parse_args()
    if a.adam2sam:
        return bench_adam2sam(a)
    if a.flagstat:
        return bench_flagstat(a)
    if a.print_tags:
        return bench_print_tags(a)
    if a.mpileup:
        return bench_mpileup(a)
    if a.realign_targets:
        return bench_realign_targets(a)
    if a.reads2ref:
        return bench_reads2ref_pages(a) if a.parquet_encoder else bench_reads2ref(a)
    if a.aggregate:
        return bench_aggregate(a)
    if a.bam_region:
        return bench_bam_region(a)
    if a.bam_out:
        return bench_bam_index(a) if a.bam_index else bench_bam_out(a)
    if a.parquet_encoder:
        return bench_transform_pages(a)
    t0 = time.perf_counter()
    data = synthetic_sam(a.reads, a.len)
    if a.bam:
        from adam_amd.bam_writer import sam_to_bam_parallel
        data = sam_to_bam_parallel(data, min(16, os.cpu_count() or 1),
                                   progress=lambda i, n: log("bam slice %d / %d" % (i, n)) if i % 8 == 0 else None)
    t_gen = time.perf_counter() - t0
    log("generated %d bytes in %.1f s" % (len(data), t_gen))
    import torch
    from adam_amd import bqsr
    from adam_amd import transform as T
    torch.zeros(1, device="cuda")
    bqsr.Context.get(0).tune(bgzf=a.bgzf)
    work = a.dir or tempfile.mkdtemp(prefix="bench_adam_")
    os.makedirs(work, exist_ok=True)
    src = os.path.join(work, "in.bam" if a.bam else "in.sam")
    with open(src, "wb") as fh:
        fh.write(data)
    n_bytes = len(data)
    header_bytes = 0 if a.bam else len(T.sam_partitions(data, len(data))[0])
    del data
    out = os.path.join(work, "out.adam")
    try:
        # warm: the first call builds the context and loads pyarrow
        log("warm-up transform")
        T.transform(src, out, mark_duplicates=not a.no_markdup, recalibrate=True,
                    partition_bytes=a.partition_bytes, compression=a.compression, part_reads=a.part_reads,
                    overwrite=True, sort_reads=a.sort_reads)
        best = None
        for _ in range(a.reps):
            log("timed transform")
            t0 = time.perf_counter()
            st = T.transform(src, out, mark_duplicates=not a.no_markdup, recalibrate=True,
                             partition_bytes=a.partition_bytes, compression=a.compression, part_reads=a.part_reads,
                             overwrite=True, sort_reads=a.sort_reads)
            dt = time.perf_counter() - t0
            if best is None or dt < best[0]:
                best = (dt, st)
        dt, st = best
        out_bytes = sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out))
        if st["reads"] != a.reads:
            raise SystemExit("transformed %d reads, expected %d" % (st["reads"], a.reads))
        print(json.dumps({
            "metric": "transform %s -> ADAM Parquet reads/s (device parse, %sBQSR, ADAM columns on the device, "
                      "part files by host threads)" % ("BAM" if a.bam else "SAM",
                                                       "" if a.no_markdup else "MarkDuplicates, "),
            "reads": a.reads, "read_len": a.len, "input_bytes": n_bytes, "output_bytes": out_bytes,
            "seconds": dt, "reads_per_s": a.reads / dt, "compression": a.compression,
            "bgzf": (("device" if a.bgzf else "host threads") if a.bam else None),
            "part_reads": a.part_reads, "partition_bytes": a.partition_bytes, "gen_seconds": t_gen,
            "sort_reads": a.sort_reads, "record_text_bytes": None if a.bam else n_bytes - header_bytes,
            "stats": {k: v for k, v in st.items()}}))
    finally:
        if not a.dir:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
