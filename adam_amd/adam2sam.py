"""`adam2sam`: ADAMRecord Parquet out as SAM or BAM.

    python -m adam_amd.adam2sam IN.adam OUT.{sam,bam} [-sort_reads] [-bam_compression_level N]
        [-bam_compressor {host,device}] [-bam_index] [-header_from FILE.{sam,bam}] [-overwrite]

The inverse of the load `transform` does (SAMRecordConverter.convert,
core/converters/SAMRecordConverter.scala:26-144): Arrow decodes the Parquet
pages on host threads, the column buffers go to the device as they are, two
kernels render every record as its SAM line (adam_lines.hip; the line's rules
and refusals: include/adam_sam.h at bqsr_arrow_sam_lines) and the text is
parsed there like SAM input (parquet.sam_text).  From there on the job is
`transform`'s: the same sort (-sort_reads), the same sinks -- SAM text, or BAM
with either compressor and -bam_index -- and their refusals.

The header is synthesised from the table (parquet.sam_header: @SQ and @RG
lines only -- ADAMRecord carries nothing of @HD, @PG or @CO), or taken as it is
from -header_from, a SAM or BAM file: the lossless round trip (original order,
unused contigs, @HD).  A record whose referenceName or mateReference is not
among that header's @SQ names is refused before anything is written.

One resident input per job: the whole table's column buffers, then its text
and the parse's columns, are on the device at once; an input that does not
fit fails with BQSRError (UNSUPPORTED) and no output appears.  Not built here:
streaming by row group, and MarkDuplicates / BQSR in this command -- run
`transform IN.adam OUT.adam` first.
"""
from __future__ import annotations

import argparse
import struct
import sys
import time
import zlib
from typing import Dict, Optional

from . import bqsr
from .inputs import Phases, is_bam, is_parquet, report
from .transform import (BAM_COMPRESSORS, BAM_INDEX_REFUSAL, BAM_PIECE_READS, DEVICE_LEVEL_REFUSAL, _BamOut, _SamOut)

COMPRESSOR_REFUSAL = "-bam_compressor applies to BAM output only (an output name ending in .bam)"


def _bam_header_text(fh) -> bytes:
    """the header text of a BAM file: its first BGZF members inflated until the text is whole"""
    raw = b""
    need = 8
    while len(raw) < need:
        head = fh.read(18)
        if len(head) < 18 or head[:4] != b"\x1f\x8b\x08\x04":
            raise ValueError("-header_from: truncated BAM header")
        size = struct.unpack_from("<H", head, 16)[0] + 1
        raw += zlib.decompress(fh.read(size - 18)[:-8], -15)
        if len(raw) >= 8:
            if raw[:4] != b"BAM\1":
                raise ValueError("-header_from: no BAM magic")
            need = 8 + struct.unpack_from("<i", raw, 4)[0]
    return raw[8:need].rstrip(b"\0")


def read_header(path: str) -> bytes:
    """The header lines of a SAM or BAM file, as they are."""
    with open(path, "rb") as fh:
        if is_bam(fh.read(4)):
            fh.seek(0)
            text = _bam_header_text(fh)
        else:
            fh.seek(0)
            lines = []
            for line in fh:
                if not line.startswith(b"@"):
                    break
                lines.append(line)
            text = b"".join(lines)
    if text and not text.endswith(b"\n"):
        text += b"\n"
    return text


def adam2sam(inp: str, out: str, sort_reads: bool = False, bam_level: Optional[int] = None,
             bam_compressor: Optional[str] = None, bam_index: bool = False, header_from: Optional[str] = None,
             overwrite: bool = False, device: int = 0, bam_piece_reads: int = BAM_PIECE_READS) -> Dict[str, float]:
    """ADAMRecord Parquet `inp` (a file or a directory of part files) written
    as SAM text, or as BAM when `out` ends in .bam (see the module doc; the
    options are `transform`'s).  Returns the stats `transform` returns:
    reads, phases (read: Arrow's decode on the host; header; lines: the
    chunk buffers, their upload, the two kernels and the parse; sort; emit;
    close), adam_lines (the split of `lines`), bam for BAM output, seconds."""
    from . import parquet as P
    bam_out = out.endswith(".bam")
    if bam_index and not bam_out:  # before anything is read
        raise ValueError(BAM_INDEX_REFUSAL)
    if bam_compressor is not None and not bam_out:
        raise ValueError(COMPRESSOR_REFUSAL)
    if bam_compressor is not None and bam_compressor not in BAM_COMPRESSORS:
        raise ValueError("-bam_compressor must be one of %s" % ", ".join(BAM_COMPRESSORS))
    if bam_compressor == "device" and bam_level is not None:
        raise ValueError(DEVICE_LEVEL_REFUSAL)
    if not is_parquet(inp):
        raise ValueError("adam2sam reads ADAM Parquet (a .adam / .parquet file or a directory of part files); "
                         "SAM and BAM input go through transform")
    t0 = time.perf_counter()
    sink = (_BamOut(out, bam_level, bam_piece_reads, overwrite, bam_compressor or "host", bam_index) if bam_out
            else _SamOut(out, overwrite))
    ok = False
    stats: Dict[str, float] = {}
    sam = None
    try:
        ctx = bqsr.Context.get(device)
        ph = Phases()
        with ph("read"):
            table = P.read_table(inp)
        with ph("header"):
            header = read_header(header_from) if header_from is not None else P.sam_header(table)
        with ph("lines"):
            sam = P.sam_text(table, header, ctx)
        del table
        stats["reads"] = sam.counts().n_reads
        stats["adam_lines"] = sam.adam_lines
        if sort_reads:
            with ph("sort"):
                sam.sort()
        with ph("emit"):
            sink.emit(0, sam, None)
        stats["phases"] = ph.t
        ok = True
    finally:
        if sam is not None:
            sam.close()
        t1 = time.perf_counter()
        sink.close(ok)
        stats.setdefault("phases", {})["close"] = time.perf_counter() - t1
    if bam_out:
        stats["bam"] = sink.stats
    stats["seconds"] = time.perf_counter() - t0
    return stats


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="adam_amd.adam2sam", description=__doc__.split("\n\n")[0])
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("-sort_reads", action="store_true", help="sort the records by reference position before the save")
    ap.add_argument("-bam_compression_level", type=int, default=None, choices=range(10), metavar="N",
                    help="BAM output: the BGZF members' DEFLATE level, 0-9 (default 6); the host compressor's")
    ap.add_argument("-bam_compressor", default=None, choices=BAM_COMPRESSORS,
                    help="BAM output: who deflates the BGZF members: host threads (default) or the device")
    ap.add_argument("-bam_index", action="store_true",
                    help="BAM output: write OUTPUT.bam.bai beside it (the output must be in coordinate order)")
    ap.add_argument("-header_from", default=None, metavar="FILE",
                    help="take the header lines of this SAM or BAM file as they are instead of synthesising them")
    ap.add_argument("-overwrite", action="store_true", help="replace an existing output file")
    a = ap.parse_args(argv)
    bam_out = a.output.endswith(".bam")
    if a.bam_compressor is not None and not bam_out:
        ap.error(COMPRESSOR_REFUSAL)
    if a.bam_compressor == "device" and a.bam_compression_level is not None:
        ap.error(DEVICE_LEVEL_REFUSAL)
    if a.bam_index and not bam_out:
        ap.error(BAM_INDEX_REFUSAL)
    t0 = time.perf_counter()
    st = adam2sam(a.input, a.output, a.sort_reads, a.bam_compression_level, a.bam_compressor, a.bam_index,
                  a.header_from, a.overwrite)
    report(st, t0)
    return 0


if __name__ == "__main__":
    sys.exit(main())
