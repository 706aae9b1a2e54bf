"""Indel realignment targets on the device: stage 1 of `transform -realignIndels`.

The reference's RealignIndels.realignIndels starts with
RealignmentTargetFinder(reads) (adam-core/.../algorithms/realignmenttarget/
RealignmentTargetFinder.scala:54-101, IndelRealignmentTarget.scala): every
read becomes its ADAMPileup rows, the rows of one position -- a rod -- become
a candidate target when they show indel evidence (I, D and S rows) or enough
mismatch quality (mismatchQuality / matchQuality >= 0.15, or no match quality
at all), and the candidates, sorted by the start of their read range, are
folded left to right: one that overlaps the last target merges into it.  Here
the pileup walk, the grouping by position, the per-rod sums, the candidates'
order and the targets' sets run on the GPU (include/adam_sam.h
``bqsr_sam_realign_targets_*`` / ``bqsr_arrow_realign_targets_*``,
adam_amd/csrc/realign_targets.hip); the serial fold runs on the host over the
candidates' (start, end) pairs only.

What is kept from the reference, quirks included:

* No LocusPredicate, for any input (Transform loads with plain adamLoad): an
  unmapped or FLAG-0 read with CIGAR and MD fails the job with PILEUP, as
  every exception of reads2ref's walk does, naming the first such read.
* Rods are keyed by position alone: equal positions on two references share a
  rod.  Soft-clipped bases are indel evidence.  The quality sums are Java Ints.
* overlap is the reference's four clauses: a candidate merges when it starts
  where the last target starts or ends, or lies inside it; a partial overlap
  starts a new target.
* A target folded from two or more candidates has one range per distinct
  indelRange (read range: the hull); a target from a single rod keeps ranges
  that differ only in their read range.

What this project declares where the reference is loose: candidates fold in
ascending (start, position) order; a target's indel ranges ascend by
(indel_start, indel_end, indel_read_start, indel_read_end), its SNP ranges by
(snp_site, snp_read_start, snp_read_end).

Stages 2 and 3 (mapTargets, realignTargetGroup) are not built;
``transform -realignIndels`` stays refused.  The reference has no printer for
targets; the text is this project's: per target ``T start end nIndel nSnp``,
its ``I indelStart indelEnd readStart readEnd`` lines, its ``S site readStart
readEnd`` lines.

    python -m adam_amd.realignment_targets INPUT.{sam,bam,adam} [-output FILE] [-targets_only]
"""
from __future__ import annotations

import argparse
import ctypes
import os
import sys
import time
from typing import Dict, Optional, Sequence

import numpy as np

from . import _capi, bqsr
from ._capi import check, dblp, vp
from .inputs import Phases, SamInput, add_region_arguments, is_parquet, region_plan, report, text_output

# the ADAMRecord columns read from Parquet: reads2ref's without the read-level
# ones it only copies and without LocusPredicate's, except readMapped, which
# the walk itself asks for
PROJECTION = ("start", "sequence", "cigar", "qual", "mismatchingPositions", "readMapped")
COLUMNS = ("target_start", "target_end", "indel_offset", "snp_offset", "indel_start", "indel_end", "indel_read_start",
           "indel_read_end", "snp_site", "snp_read_start", "snp_read_end")
KERNELS = ("count", "emit", "sort", "rods", "candidates", "fold_host", "sets")


class RealignTargetsSizes(ctypes.Structure):
    _fields_ = [("n_reads", ctypes.c_int64), ("n_rows", ctypes.c_int64), ("n_candidates", ctypes.c_int64),
                ("n_targets", ctypes.c_int64), ("n_indels", ctypes.c_int64), ("n_snps", ctypes.c_int64)]


class RealignTargetsHost(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in COLUMNS]


_SIG = {
    "bqsr_sam_realign_targets_prepare": (ctypes.c_int, [vp, vp, vp, ctypes.POINTER(RealignTargetsSizes)]),
    "bqsr_arrow_realign_targets_prepare": (ctypes.c_int, [vp, vp, vp, ctypes.POINTER(RealignTargetsSizes)]),
    "bqsr_sam_realign_targets_fetch": (ctypes.c_int, [vp, vp, ctypes.POINTER(RealignTargetsHost), vp]),
    "bqsr_arrow_realign_targets_fetch": (ctypes.c_int, [vp, vp, ctypes.POINTER(RealignTargetsHost), vp]),
    "bqsr_realign_targets_kernel_times": (ctypes.c_int, [dblp]),
}


def _lib():
    return _capi.bind(_capi.lib(), _SIG)


def kernel_times() -> Dict[str, float]:
    """ms of this thread's last prepare, by device events except ``fold_host``
    (measurement only)"""
    return _capi.stage_times(_lib().bqsr_realign_targets_kernel_times, KERNELS, array=True)


def _length(name: str, sz: RealignTargetsSizes) -> int:
    if name.startswith("target_"):
        return sz.n_targets
    if name.endswith("_offset"):
        return sz.n_targets + 1
    return sz.n_indels if name.startswith("indel_") else sz.n_snps


def _run(prepare, fetch, ctx, handle, stream=None, sizes: Optional[RealignTargetsSizes] = None) -> Dict[str, np.ndarray]:
    sz = sizes
    if sz is None:
        sz = RealignTargetsSizes()
        check(prepare(ctx.handle, handle, stream, ctypes.byref(sz)))
    H = RealignTargetsHost()
    out = {}
    for name in COLUMNS:
        a = np.zeros(_length(name, sz), np.int64)
        out[name] = a
        setattr(H, name, a.ctypes.data if a.size else None)
    check(fetch(ctx.handle, handle, ctypes.byref(H), stream))
    return out


def sam_prepare(sam, stream=None) -> RealignTargetsSizes:
    """bqsr_sam_realign_targets_prepare over a sam.SamText: the job's sizes"""
    sz = RealignTargetsSizes()
    check(_lib().bqsr_sam_realign_targets_prepare(sam.ctx.handle, sam.h, stream, ctypes.byref(sz)))
    return sz


def sam_targets(sam, stream=None, sizes: Optional[RealignTargetsSizes] = None) -> Dict[str, np.ndarray]:
    """The realignment targets of a sam.SamText's reads: a dict of int64
    arrays under the names of bqsr_realign_targets_host."""
    L = _lib()
    return _run(L.bqsr_sam_realign_targets_prepare, L.bqsr_sam_realign_targets_fetch, sam.ctx, sam.h, stream, sizes)


def arrow_prepare(reads, stream=None) -> RealignTargetsSizes:
    """bqsr_arrow_realign_targets_prepare over a parquet.ArrowReads"""
    sz = RealignTargetsSizes()
    check(_lib().bqsr_arrow_realign_targets_prepare(reads.ctx.handle, reads.h, stream, ctypes.byref(sz)))
    return sz


def arrow_targets(reads, stream=None, sizes: Optional[RealignTargetsSizes] = None) -> Dict[str, np.ndarray]:
    """As :func:`sam_targets` over a parquet.ArrowReads (its table as given:
    no LocusPredicate)."""
    L = _lib()
    return _run(L.bqsr_arrow_realign_targets_prepare, L.bqsr_arrow_realign_targets_fetch, reads.ctx, reads.h, stream,
                sizes)


def realignment_targets(path: str, device: int = 0, stats: Optional[dict] = None, region: Optional[str] = None,
                        bai: Optional[str] = None) -> Dict[str, np.ndarray]:
    """RealignmentTargetFinder over a SAM, BAM or ADAMRecord Parquet input (a
    file or a directory of part files): the targets as a dict of int64 numpy
    arrays -- ``target_start`` / ``target_end`` per target, ``indel_offset``
    / ``snp_offset`` (n_targets + 1 entries) into the ``indel_*`` and
    ``snp_*`` arrays.  Raises :class:`_capi.BQSRError` (``.read``: the read's
    index in the input) where the reference throws.  `stats`, when given,
    receives the job's sizes, phase and kernel times.  region, bai: BAM input read through its .bai index, only the reads that overlap the region (inputs.SamInput)."""
    region = region_plan(path, region, bai)  # (refused before anything is read)
    ctx = bqsr.Context.get(device)
    ph = Phases()

    def job(prepare, fetch, n_reads):
        with ph("prepare"):
            sz = prepare()
        kt = kernel_times()
        with ph("fetch"):
            out = fetch(sz)
        if stats is not None:
            stats.update(reads=n_reads, rows=sz.n_rows, candidates=sz.n_candidates, targets=sz.n_targets,
                         indels=sz.n_indels, snps=sz.n_snps, kernel_ms=kt)
        return out

    if is_parquet(path):
        from . import parquet as P
        with ph("read"):
            table = P.read_table(path, columns=PROJECTION)
        with ph("parse"):
            A = P.ArrowReads(table, ctx)
        try:
            out = job(lambda: arrow_prepare(A), lambda sz: arrow_targets(A, sizes=sz), table.num_rows)
        finally:
            A.close()
    else:
        with SamInput(path, ctx, ph, region=region, bai=bai) as src:
            for sam, _ in src:
                out = job(lambda: sam_prepare(sam), lambda sz: sam_targets(sam, sizes=sz), sam.counts().n_reads)
    if stats is not None:
        stats["phases"] = ph.t
    return out


def format_targets(t: Dict[str, np.ndarray], targets_only: bool = False) -> str:
    """The command's text of a result of :func:`realignment_targets`."""
    out = []
    io, so = t["indel_offset"], t["snp_offset"]
    for k in range(len(t["target_start"])):
        out.append("T %d %d %d %d\n" % (t["target_start"][k], t["target_end"][k], io[k + 1] - io[k], so[k + 1] - so[k]))
        if targets_only:
            continue
        for j in range(io[k], io[k + 1]):
            out.append("I %d %d %d %d\n" % (t["indel_start"][j], t["indel_end"][j], t["indel_read_start"][j],
                                            t["indel_read_end"][j]))
        for j in range(so[k], so[k + 1]):
            out.append("S %d %d %d\n" % (t["snp_site"][j], t["snp_read_start"][j], t["snp_read_end"][j]))
    return "".join(out)


def write_targets(inp: str, out: Optional[str] = None, targets_only: bool = False, device: int = 0,
                  stdout=None, region: Optional[str] = None, bai: Optional[str] = None) -> Dict[str, object]:
    """The command: the targets of `inp` as text to `out` or, without it, to
    stdout (inputs.text_output).  Returns the job's statistics."""
    stats: Dict[str, object] = {}
    region = region_plan(inp, region, bai)  # (refused before anything is read or created)
    with text_output(out, stdout) as sink:
        text = format_targets(realignment_targets(inp, device, stats, region, bai), targets_only).encode()
        sink.write(text)
    stats["bytes"] = len(text)
    return stats


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="adam_amd.realignment_targets", description=__doc__.split("\n\n")[0])
    ap.add_argument("input")
    ap.add_argument("-output", default=None, help="write the text here (default: stdout)")
    ap.add_argument("-targets_only", action="store_true", help="print only the T lines")
    add_region_arguments(ap)
    a = ap.parse_args(argv)
    if not os.path.exists(a.input):
        ap.error("no such input: %s" % a.input)
    try:
        a.region = region_plan(a.input, a.region, a.bai)
    except (ValueError, OSError) as e:
        ap.error(str(e))
    t0 = time.perf_counter()
    st = write_targets(a.input, a.output, a.targets_only, region=a.region, bai=a.bai)
    report(st, t0)
    return 0


if __name__ == "__main__":
    sys.exit(main())
