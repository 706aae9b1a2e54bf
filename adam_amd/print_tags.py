"""`adam print_tags`: tag and tag-value counts on the device
(adam-cli/.../cli/PrintTags.scala:35-91 over adamCharacterizeTags /
adamCharacterizeTagValues, adam-core/.../rdd/AdamRDDFunctions.scala:200-229,
and AttributeUtils, adam-core/.../util/AttributeUtils.scala:28-99).

    python -m adam_amd.print_tags INPUT.{sam,bam,adam,parquet} [-list N] [-count T1,T2,...] [-partition_bytes N]

prints on stdout, for the records with failedVendorQualityChecks false: with
``-list N`` the attributes of the first N of them, then a ``"%3s\\t%d"`` line
per tag, under a tag named by ``-count`` a ``"\\t%10d\\t%s"`` line per distinct
value, and ``Total: %d``; a ``reads=... phases=...`` line goes to stderr.  SAM
text streams through the device in ``inputs.sam_partitions`` partitions
(bqsr_sam_tag_counts; integer sums, so any number of partitions gives the same
result); a BAM is one parse.  ADAMRecord Parquet is read by Arrow with the
command's projection (only the columns the file has) and every record batch's
buffers go to the device as they are (bqsr_arrow_tag_counts).  Counted tags
take one more pass over the partitions -- one re-parse, every tag counted
partition by partition (bqsr_sam_tag_values / bqsr_arrow_tag_values); the host
merges the runs by (type, text).

The reference leaves its line orders to hash maps; here tags are printed
ascending by their two bytes, and values by descending count, then type letter
in the order A i f Z H, then value text ascending by bytes.  Everything is
computed first and printed only when the whole job succeeds -- the reference
would already have printed its ``-list`` lines when a later stage throws.

An attribute the reference throws at raises ``BQSRError`` ATTRIBUTE, a null
failedVendorQualityChecks or null attributes NULL_FIELD, a non-ASCII tag name
or a B value under ``-count`` UNSUPPORTED; ``.read`` is the record's ordinal in
the whole input.  There is no host fallback.
"""
from __future__ import annotations

import argparse
import ctypes
import sys
import time
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _capi, bqsr
from ._capi import check, dblp, i32, vp
from .inputs import DEFAULT_PARTITION_BYTES, Phases, SamInput, add_region_arguments, is_parquet, rebased, region_plan, report

# the command's projection (cli/PrintTags.scala:68)
PROJECTION = ("attributes", "primaryAlignment", "readMapped", "readPaired", "failedVendorQualityChecks")
TYPE_ORDER = "AifZH"
HASH_BITS = 64

ValueKey = Tuple[str, str]  # (type letter, value text as the reference prints it)


class _TagCounts(ctypes.Structure):
    """bqsr_tag_counts (include/adam_sam.h)"""
    _fields_ = [("counts", ctypes.c_int64 * (128 * 128)), ("total", ctypes.c_int64)]


class TagsChunk(ctypes.Structure):
    """bqsr_tags_chunk (include/adam_sam.h)"""
    _fields_ = [("n_reads", ctypes.c_int64), ("attr_offsets", ctypes.c_void_p), ("attr_bytes", ctypes.c_void_p),
                ("attr_validity", ctypes.c_void_p), ("failed", ctypes.c_void_p), ("failed_validity", ctypes.c_void_p)]


class _ValueSizes(ctypes.Structure):
    _fields_ = [("n_runs", ctypes.c_int64), ("text_bytes", ctypes.c_int64)]


class _ValueHost(ctypes.Structure):
    _fields_ = [("type", ctypes.c_void_p), ("count", ctypes.c_void_p), ("first_read", ctypes.c_void_p),
                ("text_offsets", ctypes.c_void_p), ("text", ctypes.c_void_p)]


KERNELS = ("scan", "values")
_SIG = {
    "bqsr_sam_tag_counts": (ctypes.c_int, [vp, vp, vp, ctypes.POINTER(_TagCounts)]),
    "bqsr_arrow_tag_counts": (ctypes.c_int, [vp, ctypes.POINTER(TagsChunk), i32, vp, ctypes.POINTER(_TagCounts)]),
    "bqsr_sam_tag_values": (ctypes.c_int, [vp, vp, ctypes.c_char_p, i32, vp, ctypes.POINTER(_ValueSizes)]),
    "bqsr_arrow_tag_values": (ctypes.c_int, [vp, ctypes.POINTER(TagsChunk), i32, ctypes.c_char_p, i32, vp,
                                             ctypes.POINTER(_ValueSizes)]),
    "bqsr_tag_values_fetch": (ctypes.c_int, [ctypes.POINTER(_ValueHost)]),
    "bqsr_tags_kernel_times": (ctypes.c_int, [dblp, dblp]),
}


def _lib():
    return _capi.bind(_capi.lib(), _SIG)


def kernel_times() -> Tuple[float, float]:
    """(scan ms, values ms) of this thread's last calls (measurement only)"""
    return tuple(_capi.stage_times(_lib().bqsr_tags_kernel_times, KERNELS).values())


def _tag_bytes(tag) -> bytes:
    """The two bytes of a tag name; ValueError otherwise (the reference's
    assert, AdamRDDFunctions.scala:222)."""
    b = tag if isinstance(tag, bytes) else tag.encode("latin-1")
    if len(b) != 2:
        raise ValueError("a tag name has two characters: %r" % (tag,))
    return b


def _counts_dict(r: _TagCounts) -> Tuple[Dict[str, int], int]:
    a = np.frombuffer(r, dtype=np.int64, count=128 * 128)
    return {chr(int(k) >> 7) + chr(int(k) & 127): int(a[k]) for k in np.flatnonzero(a)}, int(r.total)


def _add(into: Dict, more: Dict) -> None:
    for k, v in more.items():
        into[k] = into.get(k, 0) + v


def _fetch_runs(sz: _ValueSizes) -> Tuple[Dict[ValueKey, int], Dict[ValueKey, int]]:
    """The runs of the last values call merged by (type, text): (counts, first reads)"""
    n = sz.n_runs
    typ = np.zeros(max(1, n), np.uint8)
    cnt = np.zeros(max(1, n), np.int64)
    first = np.zeros(max(1, n), np.int64)
    off = np.zeros(n + 1, np.int64)
    text = np.zeros(max(1, sz.text_bytes), np.uint8)
    H = _ValueHost(typ.ctypes.data, cnt.ctypes.data, first.ctypes.data, off.ctypes.data, text.ctypes.data)
    check(_lib().bqsr_tag_values_fetch(ctypes.byref(H)))
    raw = text.tobytes()
    out: Dict[ValueKey, int] = {}
    firsts: Dict[ValueKey, int] = {}
    for r in range(n):
        t = chr(int(typ[r]))
        v = raw[off[r]:off[r + 1]].decode("latin-1")
        if t == "H":  # IndexedSeq[Byte].toString
            v = "Vector(%s)" % ", ".join(v)
        k = (t, v)
        out[k] = out.get(k, 0) + int(cnt[r])
        firsts[k] = min(firsts.get(k, int(first[r])), int(first[r]))
    return out, firsts


def sam_tag_counts(sam, stream=None) -> Tuple[Dict[str, int], int]:
    """bqsr_sam_tag_counts over a sam.SamText: ({tag: count}, kept records)"""
    r = _TagCounts()
    check(_lib().bqsr_sam_tag_counts(sam.ctx.handle, sam.h, stream, ctypes.byref(r)))
    return _counts_dict(r)


def sam_tag_values(sam, tag, hash_bits: int = HASH_BITS, stream=None) -> Dict[ValueKey, int]:
    """bqsr_sam_tag_values over a sam.SamText (not validating: see
    SamText.tag_values): {(type, text): count}"""
    sz = _ValueSizes()
    check(_lib().bqsr_sam_tag_values(sam.ctx.handle, sam.h, _tag_bytes(tag), hash_bits, stream, ctypes.byref(sz)))
    return _fetch_runs(sz)[0]


def arrow_tag_counts(chunks: Sequence[TagsChunk], ctx: Optional[bqsr.Context] = None, stream=None
                     ) -> Tuple[Dict[str, int], int]:
    """bqsr_arrow_tag_counts over TagsChunk structures (host pointers the
    caller keeps alive): ({tag: count}, kept records)"""
    ctx = ctx or bqsr.Context.get(0)
    arr = (TagsChunk * max(1, len(chunks)))(*chunks)
    r = _TagCounts()
    check(_lib().bqsr_arrow_tag_counts(ctx.handle, arr, len(chunks), stream, ctypes.byref(r)))
    return _counts_dict(r)


def arrow_tag_values(chunks: Sequence[TagsChunk], tag, ctx: Optional[bqsr.Context] = None,
                     hash_bits: int = HASH_BITS, stream=None) -> Dict[ValueKey, int]:
    """bqsr_arrow_tag_values (after arrow_tag_counts succeeded on the same chunks): {(type, text): count}"""
    ctx = ctx or bqsr.Context.get(0)
    arr = (TagsChunk * max(1, len(chunks)))(*chunks)
    sz = _ValueSizes()
    check(_lib().bqsr_arrow_tag_values(ctx.handle, arr, len(chunks), _tag_bytes(tag), hash_bits, stream,
                                       ctypes.byref(sz)))
    return _fetch_runs(sz)[0]


def table_chunks(table):
    """(chunks, keep): one TagsChunk per record batch of an Arrow table holding
    (some of) `attributes` and `failedVendorQualityChecks`, arrays normalised
    to offset 0 and large_string cast to string; an absent column is passed as
    NULL (a column of nulls).  `keep` owns the buffers."""
    import pyarrow as pa
    names = set(table.column_names)
    keep = []

    def flat(a, typ):
        if a.type != typ:
            a = a.cast(typ)
        if a.offset:
            a = pa.concat_arrays([a])
        keep.append(a)
        return a

    def addr(b):
        return None if b is None else b.address

    chunks = []
    for rb in table.to_batches():
        if rb.num_rows == 0:
            continue
        C = TagsChunk()
        C.n_reads = rb.num_rows
        if "attributes" in names:
            b = flat(rb.column(rb.schema.get_field_index("attributes")), pa.string()).buffers()
            C.attr_validity, C.attr_offsets, C.attr_bytes = addr(b[0]), addr(b[1]), addr(b[2])
        if "failedVendorQualityChecks" in names:
            b = flat(rb.column(rb.schema.get_field_index("failedVendorQualityChecks")), pa.bool_()).buffers()
            C.failed_validity, C.failed = addr(b[0]), addr(b[1])
        chunks.append(C)
    return chunks, keep


def _table_list(table, list_n: int) -> List[str]:
    """the attributes of the first list_n kept records of an Arrow table ('null' for a null)"""
    out: List[str] = []
    if list_n <= 0:
        return out
    for rb in table.to_batches():
        attrs = rb.column(rb.schema.get_field_index("attributes")).to_pylist() \
            if "attributes" in rb.schema.names else [None] * rb.num_rows
        failed = rb.column(rb.schema.get_field_index("failedVendorQualityChecks")).to_pylist()
        for a, f in zip(attrs, failed):
            if not f:  # (a null was refused by the device before this runs)
                out.append("null" if a is None else a)
                if len(out) == list_n:
                    return out
    return out


def _sam_list(sam, hdr, want: int, out: List[str]) -> None:
    """the attributes of the kept records of a parse appended to `out` until it holds `want`"""
    from .adam_save import adam_table
    n = sam.counts().n_reads
    r0 = 0
    while r0 < n and len(out) < want:
        k = min(n - r0, max(1024, 2 * (want - len(out))))
        t = adam_table(sam, r0, k, hdr)
        for a, f in zip(t.column("attributes").to_pylist(), t.column("failedVendorQualityChecks").to_pylist()):
            if not f:
                out.append("null" if a is None else a)
                if len(out) == want:
                    return
        r0 += k


def _run(path: str, list_n: Optional[int], count: Iterable[str], device: int, partition_bytes: int,
         hash_bits: int = HASH_BITS, region: Optional[str] = None, bai: Optional[str] = None):
    """(list lines, {tag: count}, {tag: {(type, text): count}}, total, stats); region, bai: BAM input read through its .bai index, only the reads that overlap the region (inputs.SamInput)"""
    region = region_plan(path, region, bai)  # (refused before anything is read)
    ctx = bqsr.Context.get(device)
    ph = Phases()
    tags: Dict[str, int] = {}
    values: Dict[str, Dict[ValueKey, int]] = {}
    lines: List[str] = []
    total = 0
    want_list = max(0, list_n or 0)
    names = [c for c in dict.fromkeys(count) if len(c) == 2]  # (any other name is no tag of the input)
    stats: Dict[str, object] = {"reads": 0}
    kernel_ms = {"scan": 0.0, "values": 0.0}  # device events, summed over the calls (measurement only)

    def timed(which):
        kernel_ms[which] += kernel_times()[which == "values"]

    if is_parquet(path):
        from . import parquet as P
        with ph("read"):
            table = P.read_table(path, columns=PROJECTION)
            chunks, keep = table_chunks(table)
        with ph("tags"):
            tags, total = arrow_tag_counts(chunks, ctx)
            timed("scan")
        with ph("values"):
            for t in names:
                if t in tags:
                    values[t] = arrow_tag_values(chunks, t, ctx, hash_bits)
                    timed("values")
        with ph("list"):
            lines = _table_list(table, want_list)
        del keep
        stats["reads"] = table.num_rows
    else:
        from .adam_save import header_info
        with SamInput(path, ctx, ph, partition_bytes, region=region, bai=bai) as src:
            if not src.bam and len(src.data):
                stats["partitions"] = src.n_partitions

            def passes(work):
                n_reads = 0
                for sam, base in src:
                    stats.update(src.region_stats or {})
                    try:
                        work(sam)
                    except _capi.BQSRError as e:
                        raise rebased(e, base) from None
                    n_reads = base + sam.counts().n_reads
                return n_reads

            def first(sam):
                nonlocal total
                with ph("tags"):
                    c, n = sam_tag_counts(sam)
                    timed("scan")
                _add(tags, c)
                total += n
                if len(lines) < want_list:  # (only as many leading partitions as needed)
                    with ph("list"):
                        _sam_list(sam, header_info(sam), want_list, lines)

            stats["reads"] = passes(first)
            counted = [t for t in names if t in tags]
            if counted:  # one more pass: every counted tag, partition by partition
                for t in counted:
                    values[t] = {}

                def second(sam):
                    with ph("values"):
                        for t in counted:
                            _add(values[t], sam_tag_values(sam, t, hash_bits))
                            timed("values")

                passes(second)
    stats["phases"] = ph.t
    stats["kernel_ms"] = kernel_ms
    return lines, tags, values, total, stats


def characterize_tags(path: str, device: int = 0, partition_bytes: Optional[int] = None) -> Dict[str, int]:
    """adamCharacterizeTags of the kept records of a SAM, BAM or ADAMRecord
    Parquet input: {tag: count} (AdamRDDFunctions.scala:200-209)."""
    return _run(path, None, (), device, DEFAULT_PARTITION_BYTES if partition_bytes is None else partition_bytes)[1]


def characterize_tag_values(path: str, tag: str, device: int = 0, partition_bytes: Optional[int] = None,
                            hash_bits: int = HASH_BITS) -> Dict[ValueKey, int]:
    """adamCharacterizeTagValues: {(type letter, value text): count} of the
    kept records' values of `tag` (AdamRDDFunctions.scala:211-219).  A tag
    whose length is not 2 raises ValueError (the reference's assert)."""
    _tag_bytes(tag)
    pb = DEFAULT_PARTITION_BYTES if partition_bytes is None else partition_bytes
    return _run(path, None, (tag,), device, pb, hash_bits)[2].get(tag, {})


def value_order(item: Tuple[ValueKey, int]):
    """descending count, then type letter in the order A i f Z H, then value text ascending by bytes"""
    (t, v), c = item
    return -c, TYPE_ORDER.index(t), v.encode("latin-1", "replace")


def format_tags(lines: Sequence[str], tags: Dict[str, int], values: Dict[str, Dict[ValueKey, int]],
                total: int) -> str:
    """The text cli/PrintTags.scala:72-88 prints (print() adds the final
    newline as println does), in this build's fixed orders."""
    out = list(lines)
    for tag in sorted(tags, key=lambda t: t.encode("latin-1", "replace")):
        out.append("%3s\t%d" % (tag, tags[tag]))
        for (t, v), c in sorted(values.get(tag, {}).items(), key=value_order):
            out.append("\t%10d\t%s" % (c, v))
    out.append("Total: %d" % total)
    return "\n".join(out)


def print_tags(path: str, list_n: Optional[int] = None, count: Iterable[str] = (), device: int = 0,
               partition_bytes: Optional[int] = None, region: Optional[str] = None, bai: Optional[str] = None) -> str:
    """The text `adam print_tags INPUT [-list list_n] [-count ...]` prints.  A
    `count` name that is not a two-char tag of the input is ignored, as in the
    reference."""
    pb = DEFAULT_PARTITION_BYTES if partition_bytes is None else partition_bytes
    lines, tags, values, total, _ = _run(path, list_n, tuple(count), device, pb, region=region, bai=bai)
    return format_tags(lines, tags, values, total)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="adam_amd.print_tags", description=__doc__.split("\n\n")[0])
    ap.add_argument("input")
    ap.add_argument("-list", type=int, default=None, metavar="N",
                    help="also list the attributes of the first N records")
    ap.add_argument("-count", default=None, metavar="T1,T2,...",
                    help="comma-separated tag names whose distinct values are printed with their counts")
    ap.add_argument("-partition_bytes", type=int, default=DEFAULT_PARTITION_BYTES,
                    help="SAM text per streamed partition, in bytes")
    add_region_arguments(ap)
    a = ap.parse_args(argv)
    try:
        a.region = region_plan(a.input, a.region, a.bai)
    except (ValueError, OSError) as e:
        ap.error(str(e))
    t0 = time.perf_counter()
    count = tuple(a.count.split(",")) if a.count is not None else ()
    lines, tags, values, total, st = _run(a.input, a.list, count, 0, a.partition_bytes, region=a.region, bai=a.bai)
    print(format_tags(lines, tags, values, total))
    report(st, t0)
    return 0


if __name__ == "__main__":
    sys.exit(main())
