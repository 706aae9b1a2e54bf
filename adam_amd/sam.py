"""SAM text through the device (include/adam_sam.h): ingest, MarkDuplicates,
and the recalibrated text back out.

``SamText(data)`` parses a whole SAM file on the device with the
SAMRecordConverter semantics ``records.read_sam`` restates
(core/converters/SAMRecordConverter.scala:26-144); ``.batch()`` returns the
columns as a RecordBatch (byte-identical to ``read_sam``);
``.mark_duplicates()`` runs MarkDuplicates (core/rdd/MarkDuplicates.scala:24-111)
over the records and updates their duplicateRead bits; ``.rewrite(job)``
puts a ResidentJob's recalibrated quality strings into the records' QUAL
fields (the output path, core/rdd/AdamRDDFunctions.scala:37-56, as SAM text);
``.flagstat()`` counts the records as `adam flagstat` does (flagstat.py);
``.pileups()`` converts them to ADAMPileup records (reads2ref.py);
``.bam_header()`` / ``.bam_records()`` encode them as BAM on the device
(bam_out.hip) and ``bgzf_compress`` cuts such a stream into BGZF members on
host threads; ``.bam_members()`` / ``bgzf_deflate`` do that on the device
(bgzf_deflate.hip).
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import numpy as np

from . import _capi, bqsr
from ._capi import check, dblp, i32, i64, i64p, pp, vp
from .inputs import is_bam
from .records import RecordBatch


class SamCounts(ctypes.Structure):
    _fields_ = [("n_reads", ctypes.c_int64), ("seq_bytes", ctypes.c_int64), ("qual_bytes", ctypes.c_int64),
                ("cigar_ops", ctypes.c_int64), ("md_bytes", ctypes.c_int64), ("text_bytes", ctypes.c_int64),
                ("n_ref_names", ctypes.c_int32), ("n_read_groups", ctypes.c_int32)]


class SamColumns(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("flags", "rg_id", "ref_index", "start", "seq_offset", "seq",
                                               "qual_offset", "qual", "cigar_offset", "cigar", "md_offset", "md")]


class BamSizes(ctypes.Structure):
    _fields_ = [("n_reads", ctypes.c_int64), ("bytes", ctypes.c_int64), ("n_floats", ctypes.c_int64)]


BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")  # the empty last member


class DupReads(ctypes.Structure):
    _fields_ = [("n_reads", ctypes.c_int64), ("read_name", ctypes.c_void_p), ("library", ctypes.c_void_p),
                ("flags", ctypes.c_void_p), ("mate_mapped", ctypes.c_void_p), ("rg_id", ctypes.c_void_p),
                ("reference_id", ctypes.c_void_p), ("start", ctypes.c_void_p), ("qual_offset", ctypes.c_void_p),
                ("qual", ctypes.c_void_p), ("cigar_offset", ctypes.c_void_p), ("cigar", ctypes.c_void_p)]


_SIG = {
    "bqsr_sam_parse": (ctypes.c_int, [vp, ctypes.c_char_p, i64, vp, pp]),
    "bqsr_bam_parse": (ctypes.c_int, [vp, ctypes.c_char_p, i64, vp, pp]),
    "bqsr_sam_destroy": (None, [vp]),
    "bqsr_sam_get_counts": (ctypes.c_int, [vp, ctypes.POINTER(SamCounts)]),
    "bqsr_sam_ref_name": (ctypes.c_char_p, [vp, i32]),
    "bqsr_sam_device_columns": (ctypes.c_int, [vp, ctypes.POINTER(SamColumns)]),
    "bqsr_sam_download": (ctypes.c_int, [vp, ctypes.POINTER(SamColumns)]),
    "bqsr_sam_rewrite_quals": (ctypes.c_int, [vp, vp, vp, vp, vp, vp, vp, i64, vp]),
    "bqsr_sam_text_download": (ctypes.c_int, [vp, ctypes.c_char_p]),
    "bqsr_mark_duplicates": (ctypes.c_int, [ctypes.POINTER(DupReads), vp]),
    "bqsr_sam_mark_duplicates": (ctypes.c_int, [vp, i64p]),
    "bqsr_sam_markdup_path": (ctypes.c_int, [vp]),
    "bqsr_sam_batch_create": (ctypes.c_int, [vp, vp, vp, i32, vp, pp]),
    "bqsr_dup_set_create": (ctypes.c_int, [vp, i64, pp]),
    "bqsr_dup_set_add": (ctypes.c_int, [vp, vp]),
    "bqsr_dup_set_finish": (ctypes.c_int, [vp, i64p]),
    "bqsr_dup_set_apply": (ctypes.c_int, [vp, i64, vp, i64p]),
    "bqsr_dup_set_destroy": (None, [vp]),
    "bqsr_sort_order": (ctypes.c_int, [vp, i64, vp, vp, vp, vp, vp]),
    "bqsr_sam_sort": (ctypes.c_int, [vp, vp, vp]),
    "bqsr_sam_bam_form": (i32, [vp]),
    "bqsr_sam_bam_prepare": (ctypes.c_int, [vp, vp, i64, i64, vp, ctypes.POINTER(BamSizes)]),
    "bqsr_sam_bam_records": (ctypes.c_int, [vp, vp, vp, vp]),
    "bqsr_sam_bam_header": (ctypes.c_int, [vp, vp, i64, i64p]),
    "bqsr_bgzf_compress": (ctypes.c_int, [vp, i64, i32, vp, i64, i64p]),
    "bqsr_bam_kernel_times": (ctypes.c_int, [dblp, dblp]),
    "bqsr_bgzf_inflate": (ctypes.c_int, [vp, ctypes.c_char_p, i64, vp, vp, i64, i64p, vp, i64, i64p]),
    "bqsr_bgzf_deflate": (ctypes.c_int, [vp, vp, i64, vp, vp, i64, i64p, i64p]),
    "bqsr_bgzf_deflate_host": (ctypes.c_int, [vp, i64, vp, i64, i64p, i64p]),
    "bqsr_sam_bam_members": (ctypes.c_int, [vp, vp, vp, vp, i64, i64p]),
    "bqsr_deflate_code_lengths": (ctypes.c_int, [vp, i32, i32, vp]),
    "bqsr_bgzf_deflate_times": (ctypes.c_int, [dblp, dblp]),
}
BAM_KERNELS = ("len", "write")
DEFLATE_KERNELS = ("deflate", "pack")


def _lib():
    return _capi.bind(_capi.lib(), _SIG)


class SamText:
    """A SAM file parsed into device columns (bqsr_sam)."""

    def __init__(self, data: bytes, ctx: Optional[bqsr.Context] = None, stream=None, bam: bool = False):
        """data: SAM text, or BAM bytes (BGZF) with bam=True -- the same
        columns either way (bqsr_bam_parse; a BAM has no text to rewrite)."""
        self.L = _lib()
        self.ctx = ctx or bqsr.Context.get(0)
        self.h = ctypes.c_void_p()
        self.bam = bam
        parse = self.L.bqsr_bam_parse if bam else self.L.bqsr_sam_parse
        # a uint8 numpy array (e.g. a view of an mmap) is passed by address
        src = ctypes.c_char_p(data.ctypes.data) if isinstance(data, np.ndarray) and data.size else data
        if isinstance(src, np.ndarray):
            src = b""
        check(parse(self.ctx.handle, src, len(data), stream, ctypes.byref(self.h)))

    @classmethod
    def adopt(cls, h: ctypes.c_void_p, ctx: bqsr.Context) -> "SamText":
        """A bqsr_sam another call of the library made (parquet.sam_text), owned from here."""
        self = cls.__new__(cls)
        self.L, self.ctx, self.h, self.bam = _lib(), ctx, h, False
        return self

    @classmethod
    def read(cls, path: str, ctx: Optional[bqsr.Context] = None) -> "SamText":
        """A .sam or .bam file (BAM by its BGZF magic)."""
        with open(path, "rb") as fh:
            data = fh.read()
        return cls(data, ctx, bam=is_bam(data))

    @property
    def bam_form(self) -> int:
        """Which BGZF inflate served the parse (bqsr_sam_bam_form): 0 not a
        BAM, 1 the host form, 2 the device form."""
        return int(self.L.bqsr_sam_bam_form(self.h))

    def counts(self) -> SamCounts:
        c = SamCounts()
        check(self.L.bqsr_sam_get_counts(self.h, ctypes.byref(c)))
        return c

    def ref_names(self) -> List[str]:
        c = self.counts()
        return [self.L.bqsr_sam_ref_name(self.h, i).decode("latin-1") for i in range(c.n_ref_names)]

    def batch(self) -> RecordBatch:
        """The columns on the host, as records.read_sam builds them."""
        c = self.counts()
        n = c.n_reads
        a = dict(flags=np.zeros(n, np.uint32), rg_id=np.zeros(n, np.int32), ref_index=np.zeros(n, np.int32),
                 start=np.zeros(n, np.int64), seq_offset=np.zeros(n + 1, np.uint64),
                 seq=np.zeros(c.seq_bytes, np.uint8), qual_offset=np.zeros(n + 1, np.uint64),
                 qual=np.zeros(c.qual_bytes, np.uint8), cigar_offset=np.zeros(n + 1, np.uint64),
                 cigar=np.zeros(c.cigar_ops, np.uint32), md_offset=np.zeros(n + 1, np.uint64),
                 md=np.zeros(c.md_bytes, np.uint8))
        cols = SamColumns(**{k: (v.ctypes.data if v.size else None) for k, v in a.items()})
        check(self.L.bqsr_sam_download(self.h, ctypes.byref(cols)))
        return RecordBatch(a["flags"], a["rg_id"], a["ref_index"], self.ref_names(), a["start"], a["seq_offset"],
                           a["seq"], a["qual_offset"], a["qual"], a["cigar_offset"], a["cigar"], a["md_offset"],
                           a["md"])

    def device_batch(self, contigs: Optional[Sequence[str]] = None, stream=None) -> ctypes.c_void_p:
        """The records as a BQSR batch packed on the device
        (bqsr_sam_batch_create; the caller owns the returned bqsr_batch*).
        contigs: the SnpTable's contig names (None: no known sites)."""
        names = self.ref_names()
        from .records import CONTIG_UNKNOWN
        lut = np.full(max(1, len(names)), CONTIG_UNKNOWN, np.int32)
        if contigs:
            pos = {c: i for i, c in enumerate(contigs)}
            for i, nm in enumerate(names):
                lut[i] = pos.get(nm, lut[i])
        bh = ctypes.c_void_p()
        check(self.L.bqsr_sam_batch_create(self.ctx.handle, self.h, lut.ctypes.data, len(names), stream,
                                           ctypes.byref(bh)))
        return bh

    def mark_duplicates(self) -> int:
        """MarkDuplicates over the records (their duplicateRead bits updated); returns the duplicate count."""
        n = ctypes.c_int64()
        check(self.L.bqsr_sam_mark_duplicates(self.h, ctypes.byref(n)))
        return int(n.value)

    def markdup_path(self) -> int:
        """Which path served the last ``mark_duplicates()``
        (bqsr_sam_markdup_path): -1 not run, 0 the device, otherwise the bits
        of why the host form did it (1 hash collision, 2 contig or position
        beyond the packed key, 4 library rank >= 4096, 8 forced)."""
        return int(self.L.bqsr_sam_markdup_path(self.h))

    def rewrite(self, job=None) -> None:
        """The output text: every record's QUAL field replaced by the
        recalibrated string a ResidentJob (adam_amd/job.py) built from this
        parse's batch() (kept when job is None); FLAG 0x400 following
        MarkDuplicates when it ran."""
        if job is None:
            check(self.L.bqsr_sam_rewrite_quals(self.ctx.handle, self.h, None, None, None, None, None, 0, None))
            return
        p = job._ptr
        check(self.L.bqsr_sam_rewrite_quals(self.ctx.handle, self.h, job.bh, p(job.out_qual), p(job.out_start),
                                            p(job.out_len), p(job.exc), job.n_exc, job.sp))

    def sort(self, stream=None) -> None:
        """`transform -sort_reads` (bqsr_sam_sort,
        core/rdd/AdamRDDFunctions.scala:63-93): the records in the
        reference's order -- mapped reads by (referenceId, start), then the
        unmapped ones, ties in input order.  Afterwards this is the parse of
        the sorted text (``text()``, ``batch()``, the ADAM columns);
        MarkDuplicates' result travels with the records."""
        check(self.L.bqsr_sam_sort(self.ctx.handle, self.h, stream))

    def flagstat(self, stream=None):
        """`adam flagstat` over the records (bqsr_sam_flagstat,
        core/rdd/FlagStat.scala:21-116): (failed, passed), each a
        flagstat.FlagStatMetrics of the eighteen counts.  duplicateRead is
        the flags column's bit: after ``mark_duplicates()`` the duplicate
        counters follow its result."""
        from .flagstat import sam_flagstat
        return sam_flagstat(self, stream)

    def tag_counts(self, stream=None):
        """`adam print_tags` over the records (bqsr_sam_tag_counts,
        core/rdd/AdamRDDFunctions.scala:200-209): ({tag: count}, kept
        records) of the records with FLAG 0x200 clear, every attribute
        validated as AttributeUtils.parseAttribute does."""
        from .print_tags import sam_tag_counts
        return sam_tag_counts(self, stream)

    def tag_values(self, tag, hash_bits: int = 64, stream=None):
        """The distinct values of `tag` among the kept records with their
        counts (bqsr_sam_tag_values, AdamRDDFunctions.scala:211-219):
        {(type letter, value text): count}.  Runs ``tag_counts()`` first, which
        validates the records.  A tag whose length is not 2 raises ValueError."""
        from .print_tags import _tag_bytes, sam_tag_values
        _tag_bytes(tag)
        self.tag_counts(stream)
        return sam_tag_values(self, tag, hash_bits, stream)

    def pileups(self, r0: int = 0, n: Optional[int] = None, stream=None):
        """`adam reads2ref` over reads [r0, r0 + n) (bqsr_sam_pileup_*,
        core/rdd/Reads2PileupProcessor.scala:34-197): their ADAMPileup records
        as a pyarrow table (adam_save.pileup_schema's columns), reads in input
        order, a read's pileups in reverse walk order.  Every read is
        converted (LocusPredicate does not apply to SAM / BAM input); a read
        the reference throws on raises BQSRError (``.read``)."""
        from .reads2ref import sam_pileups
        return sam_pileups(self, r0, n, stream=stream)

    def mpileup(self, window_bytes: Optional[int] = None, stream=None):
        """`adam mpileup` over the reads (bqsr_sam_mpileup_*,
        core/util/PileupTraversable.scala:83-281): the pileup text, as an
        iterator over windows of whole lines (bytes) of at most window_bytes
        (mpileup.DEFAULT_WINDOW_BYTES).  LocusPredicate is applied to the
        records; a read the reference throws on, a start that decreases
        inside a run of one reference and a position whose events disagree
        on the reference base raise BQSRError before the first window."""
        from . import mpileup as M
        return M.sam_mpileup(self, M.DEFAULT_WINDOW_BYTES if window_bytes is None else window_bytes, stream)

    def realignment_targets(self, stream=None):
        """RealignmentTargetFinder over the reads (bqsr_sam_realign_targets_*,
        core/algorithms/realignmenttarget/RealignmentTargetFinder.scala:54-101):
        the indel realignment targets as a dict of int64 arrays
        (realignment_targets.COLUMNS).  No LocusPredicate; a read the pileup
        walk throws on raises BQSRError."""
        from . import realignment_targets as RT
        return RT.sam_targets(self, stream)

    def bam_header(self) -> bytes:
        """The BAM header of the parse (bqsr_sam_bam_header): magic, the
        header text unchanged, the @SQ lines as the reference list."""
        n = ctypes.c_int64()
        check(self.L.bqsr_sam_bam_header(self.h, None, 0, ctypes.byref(n)))
        buf = np.zeros(max(1, n.value), np.uint8)
        check(self.L.bqsr_sam_bam_header(self.h, buf.ctypes.data, n.value, ctypes.byref(n)))
        return buf[:n.value].tobytes()

    def bam_records(self, r0: int = 0, n: Optional[int] = None, stream=None) -> np.ndarray:
        """Records [r0, r0 + n) of the current text as BAM records
        (bqsr_sam_bam_prepare / _records: encoded on the device, float tags
        final), a uint8 array.  Use after ``rewrite`` / ``sort``.  A record
        BAM cannot hold raises BQSRError (UNSUPPORTED, ``.read``)."""
        if n is None:
            n = self.counts().n_reads - r0
        sz = BamSizes()
        check(self.L.bqsr_sam_bam_prepare(self.ctx.handle, self.h, int(r0), int(n), stream, ctypes.byref(sz)))
        out = np.empty(max(1, sz.bytes), np.uint8)
        check(self.L.bqsr_sam_bam_records(self.ctx.handle, self.h, out.ctypes.data, stream))
        return out[:sz.bytes]

    def bam_members(self, r0: int = 0, n: Optional[int] = None, stream=None) -> bytes:
        """Records [r0, r0 + n) as BGZF members deflated on the device
        (bqsr_sam_bam_prepare / _members: the encoded stream never leaves the
        device, only the packed members come back).  They inflate to
        ``bam_records(r0, n)``; zero records give zero bytes; no EOF member."""
        if n is None:
            n = self.counts().n_reads - r0
        sz = BamSizes()
        check(self.L.bqsr_sam_bam_prepare(self.ctx.handle, self.h, int(r0), int(n), stream, ctypes.byref(sz)))
        return self._members(sz.bytes, stream)

    def _members(self, stream_bytes: int, stream=None) -> bytes:
        cap = stream_bytes + 64 * (stream_bytes // 65280 + 1)
        out = np.empty(cap, np.uint8)
        got = ctypes.c_int64()
        check(self.L.bqsr_sam_bam_members(self.ctx.handle, self.h, stream, out.ctypes.data, cap, ctypes.byref(got)))
        return out[:got.value].tobytes()

    def text(self) -> bytes:
        n = self.counts().text_bytes
        buf = ctypes.create_string_buffer(max(1, n))
        check(self.L.bqsr_sam_text_download(self.h, buf))
        return buf.raw[:n]

    def close(self):
        if self.h:
            self.L.bqsr_sam_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bgzf_inflate(data: bytes, ctx: Optional[bqsr.Context] = None, stream=None):
    """The device BGZF inflate alone (bqsr_bgzf_inflate): (out, status) --
    the inflated stream as a uint8 array, member i's bytes at the sum of the
    ISIZE fields before it, and the members' status (int32; 0: inflated and
    CRC32 checked, non-zero: declined, its bytes unspecified)."""
    L = _lib()
    ctx = ctx or bqsr.Context.get(0)
    n, nb = ctypes.c_int64(), ctypes.c_int64()
    check(L.bqsr_bgzf_inflate(ctx.handle, data, len(data), stream, None, 0, ctypes.byref(n), None, 0,
                              ctypes.byref(nb)))
    out = np.zeros(max(1, n.value), np.uint8)
    status = np.full(max(1, nb.value), -1, np.int32)
    check(L.bqsr_bgzf_inflate(ctx.handle, data, len(data), stream, out.ctypes.data, n.value, ctypes.byref(n),
                              status.ctypes.data, nb.value, ctypes.byref(nb)))
    return out[:n.value], status[:nb.value]


def bgzf_compress(data, level: int = 6) -> bytes:
    """BGZF members of a byte stream (bqsr_bgzf_compress: 65280 bytes each,
    compressed by host threads; level 0: stored).  No EOF member: append
    BGZF_EOF once at the end of the file."""
    L = _lib()
    a = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
    n = int(a.size)
    cap = n + 64 * (n // 65280 + 1)
    out = np.empty(cap, np.uint8)
    got = ctypes.c_int64()
    check(L.bqsr_bgzf_compress(a.ctypes.data if n else None, n, int(level), out.ctypes.data, cap, ctypes.byref(got)))
    return out[:got.value].tobytes()


def _bytes_array(data):
    return np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)


def bgzf_deflate(data, ctx: Optional[bqsr.Context] = None, stream=None) -> bytes:
    """BGZF members of a byte stream, deflated on the device
    (bqsr_bgzf_deflate): cut as ``bgzf_compress`` cuts it, one level, the
    bytes a function of the input alone.  No EOF member."""
    L = _lib()
    ctx = ctx or bqsr.Context.get(0)
    a = _bytes_array(data)
    n = int(a.size)
    cap = n + 64 * (n // 65280 + 1)
    out = np.empty(cap, np.uint8)
    got = ctypes.c_int64()
    check(L.bqsr_bgzf_deflate(ctx.handle, a.ctypes.data if n else None, n, stream, out.ctypes.data, cap,
                              ctypes.byref(got), None))
    return out[:got.value].tobytes()


def bgzf_deflate_host(data) -> bytes:
    """``bgzf_deflate``'s bytes from the member routine compiled for the host
    (bqsr_bgzf_deflate_host: no device; for tests, slow)."""
    L = _lib()
    a = _bytes_array(data)
    n = int(a.size)
    cap = n + 64 * (n // 65280 + 1)
    out = np.empty(cap, np.uint8)
    got = ctypes.c_int64()
    check(L.bqsr_bgzf_deflate_host(a.ctypes.data if n else None, n, out.ctypes.data, cap, ctypes.byref(got), None))
    return out[:got.value].tobytes()


def deflate_code_lengths(freq, max_bits: int) -> np.ndarray:
    """The code lengths the device encoder gives a histogram
    (bqsr_deflate_code_lengths; host only): a uint8 array, 0 for an unused
    symbol.  More than 2^max_bits symbols raise BQSRError (INVALID_ARG)."""
    L = _lib()
    f = np.ascontiguousarray(freq, np.uint32)
    out = np.zeros(max(1, f.size), np.uint8)
    check(L.bqsr_deflate_code_lengths(f.ctypes.data if f.size else None, int(f.size), int(max_bits), out.ctypes.data))
    return out[:f.size]


def bgzf_deflate_times():
    """(member kernel ms, pack kernel ms) of this thread's last device deflate (measurement only)"""
    return tuple(_capi.stage_times(_lib().bqsr_bgzf_deflate_times, DEFLATE_KERNELS).values())


def bam_kernel_times():
    """(pass 1 ms, pass 2 ms) of this thread's last ``bam_records`` (measurement only)"""
    return tuple(_capi.stage_times(_lib().bqsr_bam_kernel_times, BAM_KERNELS).values())


class DupSet:
    """MarkDuplicates across the partitions of one input (bqsr_dup_set):
    add() every partition's parse in input order, finish(), then apply(i,
    parse) to a re-parse of partition i."""

    def __init__(self, ctx: Optional[bqsr.Context] = None, reads_hint: int = 0):
        self.L = _lib()
        self.ctx = ctx or bqsr.Context.get(0)
        self.h = ctypes.c_void_p()
        check(self.L.bqsr_dup_set_create(self.ctx.handle, int(reads_hint), ctypes.byref(self.h)))
        self.parts = 0

    def add(self, sam: SamText) -> int:
        check(self.L.bqsr_dup_set_add(self.h, sam.h))
        self.parts += 1
        return self.parts - 1

    def finish(self) -> int:
        n = ctypes.c_int64()
        check(self.L.bqsr_dup_set_finish(self.h, ctypes.byref(n)))
        return int(n.value)

    def apply(self, part: int, sam: SamText) -> int:
        n = ctypes.c_int64()
        check(self.L.bqsr_dup_set_apply(self.h, int(part), sam.h, ctypes.byref(n)))
        return int(n.value)

    def close(self):
        if self.h:
            self.L.bqsr_dup_set_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sort_order(flags, reference_id, start, ctx: Optional[bqsr.Context] = None) -> np.ndarray:
    """bqsr_sort_order over host columns (uploaded; the order comes back to
    the host): order[i] = the input index of the read at sorted position i.
    flags: the records' flag words (BQSR_F_MAPPED = readMapped;
    BQSR_F_HAS_START unset = a null start); reference_id: -1 = null."""
    import torch
    L = _lib()
    ctx = ctx or bqsr.Context.get(0)
    n = len(flags)
    dev = torch.device("cuda", ctx.device)
    f = torch.from_numpy(np.ascontiguousarray(flags, np.uint32).view(np.int32)).to(dev)
    r = torch.from_numpy(np.ascontiguousarray(reference_id, np.int32)).to(dev)
    s = torch.from_numpy(np.ascontiguousarray(start, np.int64)).to(dev)
    order = torch.empty(max(1, n), dtype=torch.int32, device=dev)
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(L.bqsr_sort_order(ctx.handle, n, f.data_ptr(), r.data_ptr(), s.data_ptr(), order.data_ptr(), sp))
    return order[:n].cpu().numpy().view(np.uint32).astype(np.int64)


def mark_duplicates(read_name: Sequence[Optional[str]], library: Sequence[Optional[str]], flags, mate_mapped,
                    rg_id, reference_id, start, qual_offset, qual, cigar_offset, cigar) -> np.ndarray:
    """bqsr_mark_duplicates over host columns (no device needed): the
    duplicateRead value MarkDuplicates gives each read."""
    L = _lib()
    n = len(flags)
    names = [None if s is None else s.encode("latin-1") for s in read_name]
    libs = [None if s is None else s.encode("latin-1") for s in library]
    name_a = (ctypes.c_char_p * max(1, n))(*names) if n else (ctypes.c_char_p * 1)()
    lib_a = (ctypes.c_char_p * max(1, n))(*libs) if n else (ctypes.c_char_p * 1)()
    arrs = dict(flags=np.ascontiguousarray(flags, np.uint32), mate_mapped=np.ascontiguousarray(mate_mapped, np.uint8),
                rg_id=np.ascontiguousarray(rg_id, np.int32), reference_id=np.ascontiguousarray(reference_id, np.int32),
                start=np.ascontiguousarray(start, np.int64), qual_offset=np.ascontiguousarray(qual_offset, np.uint64),
                qual=np.ascontiguousarray(qual, np.uint8), cigar_offset=np.ascontiguousarray(cigar_offset, np.uint64),
                cigar=np.ascontiguousarray(cigar, np.uint32))
    keep = {k: (v if v.size else np.zeros(1, v.dtype)) for k, v in arrs.items()}
    R = DupReads(n, ctypes.cast(name_a, ctypes.c_void_p), ctypes.cast(lib_a, ctypes.c_void_p),
                 *[keep[k].ctypes.data for k in ("flags", "mate_mapped", "rg_id", "reference_id", "start",
                                                  "qual_offset", "qual", "cigar_offset", "cigar")])
    dup = np.zeros(max(1, n), np.uint8)
    check(L.bqsr_mark_duplicates(ctypes.byref(R), dup.ctypes.data))
    return dup[:n].astype(bool)
