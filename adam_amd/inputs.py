"""What every command does around its own work: open the input and parse it
(:class:`SamInput`), name a read of a later partition by its ordinal in the
whole input (:func:`rebased`), write text that appears only on success
(:func:`text_output`), time the phases (:class:`Phases`) and print the closing
stats line (:func:`report`).  A new command starts from here.
"""
from __future__ import annotations

import contextlib
import mmap
import os
import sys
import time
from typing import Dict, List, Tuple

import numpy as np

from . import _capi

DEFAULT_PARTITION_BYTES = 8 << 30  # SAM text per partition: ~3x that in HBM while parsed (288 GB per GPU)


def sam_partitions(data, partition_bytes: int) -> Tuple[bytes, List[Tuple[int, int]]]:
    """(header, ranges): the SAM header lines and the byte ranges [a, b) of
    the records, each range cut after the first newline at or beyond
    partition_bytes from its start (so every record lies in one range)."""
    n = len(data)
    pos = 0
    while pos < n and data[pos:pos + 1] == b"@":
        nl = data.find(b"\n", pos)
        pos = n if nl < 0 else nl + 1
    ranges = []
    a = pos
    step = max(1, int(partition_bytes))
    while a < n:
        b = min(n, a + step)
        if b < n:
            nl = data.find(b"\n", b - 1)
            b = n if nl < 0 else nl + 1
        ranges.append((a, b))
        a = b
    return bytes(data[:pos]), ranges


def is_parquet(path: str) -> bool:
    """ADAM's own format: a Parquet file (magic PAR1) or a directory of part
    files (what adamSave writes), or a .adam / .parquet name."""
    if path.endswith((".adam", ".parquet")) or os.path.isdir(path):
        return True
    try:
        with open(path, "rb") as fh:
            return fh.read(4) == b"PAR1"
    except OSError:
        return False


class Phases:
    """wall time per named phase (the stats' phase split)"""

    def __init__(self):
        self.t: Dict[str, float] = {}

    def __call__(self, name: str):
        @contextlib.contextmanager
        def cm():
            t0 = time.perf_counter()
            try:
                yield
            finally:
                self.t[name] = self.t.get(name, 0.0) + time.perf_counter() - t0
        return cm()


def host_bytes(data):
    """the input as a bytes-like object ctypes can pass without a copy: a
    read-only mmap is passed as a numpy view's address"""
    if isinstance(data, mmap.mmap):
        return np.frombuffer(data, np.uint8)
    return data


def is_bam(data) -> bool:
    return bytes(data[:4]) == b"\x1f\x8b\x08\x04"


class SamInput:
    """A SAM or BAM file mapped read-only and parsed partition by partition:

        with SamInput(path, ctx, phases, partition_bytes) as src:
            for sam, base in src:
                ...

    `sam` is the partition's parse (a sam.SamText built under
    ``phases("parse")``), `base` the number of reads in the partitions before
    it.  SAM text longer than partition_bytes is cut by :func:`sam_partitions`
    and every range parsed with the header; a BAM, an empty file and
    partition_bytes None are one partition holding the whole input, passed
    without a copy.  One parse is open at a time: the previous one is closed
    before the next is built, the last one when the iteration ends, and
    whatever is open when the block is left -- so a failing loop body has
    released the parse's device memory and the map before its exception leaves
    the ``with``.  Every iteration parses again.

    ``.bam``, ``.n_partitions``, and ``.data`` / ``.header`` / ``.ranges``
    (the map and its cut; ranges is None for one partition) are set on entry.
    parse(data, ctx, bam=...) replaces sam.SamText; its result needs only
    ``.close()`` and ``.counts().n_reads``.

    region (``NAME``, ``NAME:BEG`` or ``NAME:BEG-END``, bam_index.parse_region)
    (or a :class:`RegionPlan` made before) reads a BAM through its .bai index
    (`bai`, else IN.bam.bai, else IN.bai):
    one partition, partition_bytes ignored, whose parse is the header plus the
    records that overlap the region, in file order; only the BGZF members the
    index names are read (bam_index.region_text; its counts are in
    ``.region_stats`` after the iteration).  :func:`region_plan` refuses on
    entry, before anything is parsed: SAM or Parquet input, a missing index, a
    reference the header does not have (ValueError)."""

    def __init__(self, path: str, ctx, phases, partition_bytes=None, parse=None, *, region=None, bai=None):
        if parse is None:
            from .sam import SamText as parse
        self.path, self.ctx, self.phases, self.partition_bytes, self.parse = path, ctx, phases, partition_bytes, parse
        self.region, self.bai = region, bai
        self.plan = None
        self.region_stats = None
        self.data = None
        self._sam = None

    def __enter__(self):
        self.plan = region_plan(self.path, self.region, self.bai)
        with open(self.path, "rb") as fh:
            self.data = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ) if os.path.getsize(self.path) else b""
        try:
            self.bam = is_bam(self.data)
            self.header = self.ranges = None
            if self.partition_bytes is not None and not self.bam and len(self.data) and self.plan is None:
                header, ranges = sam_partitions(self.data, self.partition_bytes)
                if len(ranges) > 1:
                    self.header, self.ranges = header, ranges
            self.n_partitions = len(self.ranges) if self.ranges else 1
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        try:
            self._close_parse()
        finally:
            if isinstance(self.data, mmap.mmap):
                self.data.close()
            self.data = None

    def _close_parse(self):
        sam, self._sam = self._sam, None
        if sam is not None:
            sam.close()

    def __iter__(self):
        # (no try / finally here: a generator's runs only once the traceback of a failing loop body is released)
        base = 0
        for k in range(self.n_partitions):
            self._close_parse()
            with self.phases("parse"):
                # (the view of the map is made inside the call, so that it does not outlive it)
                if self.plan is not None:
                    from .bam_index import region_text
                    self._sam, self.region_stats = region_text(self.data, self.ctx, *self.plan)
                elif self.ranges is None:
                    self._sam = self.parse(host_bytes(self.data), self.ctx, bam=self.bam)
                else:
                    a, b = self.ranges[k]
                    self._sam = self.parse(self.header + bytes(self.data[a:b]), self.ctx, bam=self.bam)
            yield self._sam, base
            base += self._sam.counts().n_reads
        self._close_parse()


class RegionPlan(tuple):
    """(index, refID, beg, end): what :func:`region_plan` made of ``-region R [-bai F]``, for bam_index.region_text"""


def region_plan(path: str, region, bai=None):
    """What ``-region R [-bai F]`` on the input at `path` reads: None without
    a region, else a :class:`RegionPlan`.  A plan given as `region` is returned
    as it is, so a command makes it once (its ``main``, or its library
    function) and hands it down as ``region=``: the header is inflated and the
    .bai read and checked one time.
    ValueError, with no device touched and nothing created, for SAM or Parquet
    input, a missing index file, a reference the BAM header does not have, a
    region that does not parse, an index that is not this file's, a BAM whose
    header does not inflate."""
    if isinstance(region, RegionPlan):
        return region
    if region is None:
        if bai is not None:
            raise ValueError("-bai goes with -region")
        return None
    from . import bam_index as BI
    if is_parquet(path):
        raise ValueError("-region reads a BAM through its .bai index: %s is Parquet input" % path)
    with open(path, "rb") as fh:
        if not is_bam(fh.read(4)):
            raise ValueError("-region reads a BAM through its .bai index: %s is not a BAM" % path)
        bai_path = BI.find_index(path, bai)
        data = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)
    try:
        _text, names, _lens = BI.bam_header(data)
        size = len(data)
    finally:
        data.close()
    rid, beg, end = BI.parse_region(region, names)
    index = BI.BaiIndex.read(bai_path)
    index.validate(len(names), size)
    return RegionPlan((index, rid, beg, end))


def add_region_arguments(ap) -> None:
    """``-region R [-bai F]`` on a command that opens its input through SamInput"""
    ap.add_argument("-region", default=None, metavar="NAME[:BEG[-END]]",
                    help="BAM input only: read the reads that overlap the region (1-based, inclusive) through the "
                         "file's .bai index (python -m adam_amd.bam_index IN.bam writes one); the command sees "
                         "exactly those reads, as if the input were the filtered file: MarkDuplicates and BQSR "
                         "(transform) work on what the region holds, and a mate outside the region is absent")
    ap.add_argument("-bai", default=None, metavar="FILE", help="the index file (default: IN.bam.bai, else IN.bai)")


def rebased(e: _capi.BQSRError, base: int) -> _capi.BQSRError:
    """e of a later partition with the read's ordinal in the whole input, in
    .read and in the message (which names the read once, as ``read N``)"""
    if e.read < 0 or not base:
        return e
    msg = str(e).split(": ", 1)[1].replace("read %d" % e.read, "read %d" % (e.read + base), 1)
    return _capi.BQSRError(e.status, msg, e.read + base)


class _Partial:
    """OUT.partial.<pid>, created at the first write"""

    def __init__(self, path: str):
        self.path = path
        self.fh = None

    def write(self, data):
        if self.fh is None:
            self.fh = open(self.path, "wb")
        return self.fh.write(data)

    def close(self):
        self.write(b"")
        self.fh.close()


@contextlib.contextmanager
def text_output(out, stdout=None):
    """A writable binary sink for a command's text.  With `out` the bytes go
    to ``OUT.partial.<pid>`` (created at the first write, or at a clean exit
    without one), which is renamed over `out` on a clean exit and removed on
    an exception: `out` appears only when the job succeeded, and a job that
    fails before it writes leaves no file at any time.  A directory as `out`
    is refused first.  Without `out` the sink is `stdout` (default: the
    process's, as bytes), flushed on a clean exit only."""
    if out is not None and os.path.isdir(out):
        raise IsADirectoryError("output path %s is a directory" % out)
    if out is None:
        sink = stdout or getattr(sys.stdout, "buffer", sys.stdout)
        yield sink
        sink.flush()
        return
    sink = _Partial("%s.partial.%d" % (out, os.getpid()))
    try:
        yield sink
        sink.close()
        os.replace(sink.path, out)
    except BaseException:
        if sink.fh is not None:
            sink.fh.close()
        if os.path.lexists(sink.path):
            os.unlink(sink.path)
        raise


def report(stats: dict, t0: float) -> None:
    """a command's closing line on stderr: the stats as ``key=value``, ``seconds`` the wall time since t0"""
    stats["seconds"] = time.perf_counter() - t0
    print(" ".join("%s=%s" % kv for kv in stats.items()), file=sys.stderr)
