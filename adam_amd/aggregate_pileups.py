"""`adam aggregate_pileups` on the device: ADAMPileup rows aggregated by position.

The reference's PileupAggregator command (adam-cli/.../cli/PileupAggregator.
scala:27-57) loads ADAMPileup records and runs PileupAggregator.aggregate
(adam-core/.../rdd/PileupAggregator.scala:25-219) "to reduce storage cost";
``reads2ref -aggregate`` runs the same over the pileups it has just made.  Here
every row is kept on the GPU as columns and one resident aggregation does the
work (include/adam_sam.h ``bqsr_pileup_agg_*``, adam_amd/csrc/pileup_agg.hip):
a key pass, a stable multi-key radix sort, and the reference's fold as two
segmented scans.  The numeric columns of the groups come back as Arrow buffers;
the string columns are joined on the host from the fetched row order.

INPUT is either ADAMPileup Parquet (a file or a part-file directory: the
reference's command), or SAM, BAM or ADAMRecord Parquet: the reads are expanded
as ``reads2ref`` does and their rows go from the emit pass into the
aggregation without leaving the device, so the result equals aggregating
``reads2ref``'s own output.

What the reference leaves to Spark's shuffle and to a hash map is DECLARED
here (and in the header):

* fold order: rows fold in input row order;
* output order: groups ascend by (referenceId, position, readBase ordinal,
  rangeOffset, recordGroupSample in byte order), integers signed, nulls first
  in every component.

Everything else is the reference's, quirks included: the accumulator's quality
is multiplied by its accumulated count (so the result depends on the fold order
and wraps mod 2^32 in deep groups), a group of one row still has its qualities
divided by its count (aggregating twice divides twice), a null read name in a
group of two or more prints as ``null``, the string recordGroup fields join
their distinct values pairwise (``X, X, Y, X`` gives ``X,Y,X``), and the two
numeric ones are null unless the accumulator and the next row agree.  Where the
reference throws the job fails and no output appears (:class:`_capi.BQSRError`,
``.read`` = the input row): NULL_FIELD for a null referenceId or position, for
a null mapQuality, sangerQuality or countAtPosition, and in groups of two or
more for a null numSoftClipped, numReverseStrand, readStart or readEnd; PILEUP
for a group whose count sums to 0.  So ``reads2ref`` output made from Parquet
reads without ``mapq`` fails here, as it would in the reference.

Not reproduced: the ``validate`` flag (never true from the CLI) and the reducer
count.  The reference's command binds LocusPredicate to the pileup file; the
predicate names ADAMRecord columns, which a pileup file lacks, and what Parquet
1.2.5 does then cannot be run here: this build applies NO predicate to pileup
input, and applies LocusPredicate to ADAMRecord Parquet input exactly as
``reads2ref.locus_filter`` does.

The whole input is one resident aggregation: at most 2^31 - 1 rows, about 72
bytes of HBM per row plus the sort's scratch while it runs.

    python -m adam_amd.aggregate_pileups INPUT OUTPUT.adam [-parquet_compression gzip|snappy|none]
        [-part_rows N] [-partition_bytes N] [-overwrite]
"""
from __future__ import annotations

import argparse
import ctypes
import sys
import time
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _capi, bqsr
from . import reads2ref as R
from ._capi import check, dblp, i64, pp, vp
from .adam_save import (BASES, PILEUP_DICT_COLS, PILEUP_FIELDS, PILEUP_STATS_COLS, RG_TAGS, AdamWriter, check_out,
                        header_info, pileup_schema)
from .inputs import DEFAULT_PARTITION_BYTES, Phases, SamInput, add_region_arguments, is_parquet, rebased, region_plan, report

DEFAULT_PART_ROWS = 1 << 20  # aggregated rows per part file (their joined read names stay far below 2 GB)
WORKGROUP = 256              # rows per scan tile (pileup_agg.hip kThreads): the size the boundary tests straddle
_ADD_ROWS = 1 << 24          # rows per add of pileup input
_TABLE_THREADS = 4           # host threads building the parts' tables ahead of the writer

RG_NUMBER = ["recordGroupRunDateEpoch", "recordGroupPredictedMedianInsertSize"]
RG_FIELDS = [n for n, _ in PILEUP_FIELDS if n.startswith("recordGroup")]

# bqsr_pileup_agg_rows' value columns, in order: (field, ADAMPileup column, dtype)
_ROWS = (("reference_id", "referenceId", np.int32), ("position", "position", np.int64),
         ("range_offset", "rangeOffset", np.int32), ("range_length", "rangeLength", np.int32),
         ("reference_base", "referenceBase", np.uint8), ("read_base", "readBase", np.uint8),
         ("sanger_quality", "sangerQuality", np.int32), ("map_quality", "mapQuality", np.int32),
         ("num_soft_clipped", "numSoftClipped", np.int32), ("num_reverse_strand", "numReverseStrand", np.int32),
         ("count_at_position", "countAtPosition", np.int32), ("read_start", "readStart", np.int64),
         ("read_end", "readEnd", np.int64), ("sample_code", None, np.int32))
# bqsr_pileup_agg_host: (field, dtype, "g" per group / "g1" groups + 1 / "r" per row / "w" per bitmap word)
_HOST = (("reference_id", np.int32, "g"), ("position", np.int64, "g"), ("range_offset", np.int32, "g"),
         ("range_length", np.int32, "g"), ("reference_base", np.uint8, "g"), ("read_base", np.uint8, "g"),
         ("sanger_quality", np.int32, "g"), ("map_quality", np.int32, "g"), ("num_soft_clipped", np.int32, "g"),
         ("num_reverse_strand", np.int32, "g"), ("count_at_position", np.int32, "g"), ("read_start", np.int64, "g"),
         ("read_end", np.int64, "g"), ("first_row", np.uint32, "g"), ("offsets", np.uint32, "g1"),
         ("order", np.uint32, "r"), ("names", np.int32, "r"), ("range_offset_valid", np.uint64, "w"),
         ("range_length_valid", np.uint64, "w"), ("reference_base_valid", np.uint64, "w"),
         ("read_base_valid", np.uint64, "w"), ("num_soft_clipped_valid", np.uint64, "w"),
         ("num_reverse_strand_valid", np.uint64, "w"), ("read_start_valid", np.uint64, "w"),
         ("read_end_valid", np.uint64, "w"), ("uniform_rg", np.uint64, "w"))


class AggRows(ctypes.Structure):
    _fields_ = ([("n_rows", ctypes.c_int64)] + [(f, ctypes.c_void_p) for f, _, _ in _ROWS] +
                [("rg_code", ctypes.c_void_p), ("name_code", ctypes.c_void_p)] +
                [(f + "_valid", ctypes.c_void_p) for f, _, _ in _ROWS])


class AggSizes(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_int64), ("n_groups", ctypes.c_int64), ("bitmap_words", ctypes.c_int64)]


class AggHost(ctypes.Structure):
    _fields_ = [(f, ctypes.c_void_p) for f, _, _ in _HOST]


KERNELS = ("keys", "sort", "scans", "emit")
_SIG = {
    "bqsr_pileup_agg_create": (ctypes.c_int, [vp, pp]),
    "bqsr_pileup_agg_destroy": (None, [vp]),
    "bqsr_pileup_agg_add_host": (ctypes.c_int, [vp, ctypes.POINTER(AggRows), vp]),
    "bqsr_sam_pileup_agg_add": (ctypes.c_int, [vp, vp, vp, vp, vp, i64, vp]),
    "bqsr_arrow_pileup_agg_add": (ctypes.c_int, [vp, vp, vp, vp, vp, i64, vp]),
    "bqsr_pileup_agg_run": (ctypes.c_int, [vp, vp, ctypes.POINTER(AggSizes)]),
    "bqsr_pileup_agg_fetch": (ctypes.c_int, [vp, ctypes.POINTER(AggHost), vp]),
    "bqsr_pileup_agg_kernel_times": (ctypes.c_int, [dblp, dblp, dblp, dblp]),
}


def _lib():
    return _capi.bind(_capi.lib(), _SIG)


def kernel_times() -> Dict[str, float]:
    """device-event times (ms) of this thread's last run: keys, sort, scans,
    emit (measurement only)"""
    return _capi.stage_times(_lib().bqsr_pileup_agg_kernel_times, KERNELS)


class Aggregation:
    """A bqsr_pileup_agg handle: every added row stays on the device."""

    def __init__(self, ctx=None):
        self.ctx = ctx or bqsr.Context.get(0)
        self.L = _lib()
        self.h = ctypes.c_void_p()
        check(self.L.bqsr_pileup_agg_create(self.ctx.handle, ctypes.byref(self.h)))
        self.n_rows = 0

    def close(self):
        if self.h:
            self.L.bqsr_pileup_agg_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def add_host(self, n_rows: int, cols: Dict[str, np.ndarray], valid: Optional[Dict[str, np.ndarray]] = None,
                 stream=None):
        """n_rows rows from host columns: cols by bqsr_pileup_agg_rows' field
        names (an absent value column is a column of nulls; rg_code is
        required), valid: Arrow validity bitmaps (uint8) by the same names."""
        valid = valid or {}
        A = AggRows()
        A.n_rows = n_rows
        keep = []
        for f, dt in [(f, dt) for f, _, dt in _ROWS] + [("rg_code", np.int32), ("name_code", np.int32)]:
            if f in cols and cols[f] is not None:
                a = np.ascontiguousarray(cols[f], dt)
                assert len(a) >= n_rows, f
                keep.append(a)
                setattr(A, f, a.ctypes.data)
            if valid.get(f) is not None:
                v = np.ascontiguousarray(valid[f], np.uint8)
                assert len(v) >= (n_rows + 7) // 8, f
                keep.append(v)
                setattr(A, f + "_valid", v.ctypes.data)
        check(self.L.bqsr_pileup_agg_add_host(self.h, ctypes.byref(A), stream))
        self.n_rows += n_rows

    def add_sam(self, sam, n_rows: int, sample_code: np.ndarray, rg_code: np.ndarray, name_base: int, stream=None):
        """the rows of the last bqsr_sam_pileup_prepare on `sam`"""
        s, g = np.ascontiguousarray(sample_code, np.int32), np.ascontiguousarray(rg_code, np.int32)
        check(self.L.bqsr_sam_pileup_agg_add(self.ctx.handle, sam.h, self.h, s.ctypes.data, g.ctypes.data, name_base,
                                             stream))
        self.n_rows += n_rows

    def add_arrow(self, reads, n_rows: int, sample_code: np.ndarray, rg_code: np.ndarray, name_base: int,
                  stream=None):
        """the rows of the last bqsr_arrow_pileup_prepare on `reads`"""
        s, g = np.ascontiguousarray(sample_code, np.int32), np.ascontiguousarray(rg_code, np.int32)
        check(self.L.bqsr_arrow_pileup_agg_add(self.ctx.handle, reads.h, self.h, s.ctypes.data, g.ctypes.data,
                                               name_base, stream))
        self.n_rows += n_rows

    def run(self, stream=None) -> AggSizes:
        sz = AggSizes()
        check(self.L.bqsr_pileup_agg_run(self.h, stream, ctypes.byref(sz)))
        return sz

    def fetch(self, sz: AggSizes, stream=None) -> Dict[str, np.ndarray]:
        """the last run's result as numpy arrays, by bqsr_pileup_agg_host's field names"""
        count = {"g": sz.n_groups, "g1": sz.n_groups + 1, "r": sz.n_rows, "w": sz.bitmap_words}
        H = AggHost()
        out = {}
        for f, dt, kind in _HOST:
            a = np.zeros(max(1, count[kind]), dt)
            out[f] = a[:count[kind]]
            setattr(H, f, a.ctypes.data)
        check(self.L.bqsr_pileup_agg_fetch(self.h, ctypes.byref(H), stream))
        return out


# ---- the host side: codes in, strings out ----------------------------------


def sample_ranks(samples: Sequence[Optional[str]]) -> np.ndarray:
    """per entry the rank of its string among the distinct ones in byte
    order, -1 for None"""
    order = {s: i for i, s in enumerate(sorted({s for s in samples if s is not None}, key=lambda s: s.encode()))}
    return np.array([-1 if s is None else order[s] for s in samples], np.int32).reshape(-1)


class Units:
    """What the string columns of the groups are made from.  A unit is what a
    row's name code points at: a read (read input) or a row (pileup input).
    names: Arrow string arrays, concatenated in unit order; ref_code: per unit
    the index into ref_values (-1: null); rg_code: per unit the index into the
    per-code value lists of rg_values (by ADAMPileup column)."""

    def __init__(self):
        self.names: List = []
        self.ref_code: List[np.ndarray] = []
        self.rg_code: List[np.ndarray] = []
        self.ref_values: List[Optional[str]] = []
        self.rg_values: Dict[str, list] = {f: [None] for f in RG_FIELDS}
        self.n = 0

    def add(self, names, ref_code, rg_code):
        self.names.append(names)
        self.ref_code.append(np.asarray(ref_code, np.int32))
        self.rg_code.append(np.asarray(rg_code, np.int32))
        self.n += len(names)

    def freeze(self):
        import pyarrow as pa
        # one array: a take from a chunked array concatenates its chunks on every call
        self.all_names = (pa.concat_arrays([c.cast(pa.large_string()) for c in self.names]) if self.names
                          else pa.array([], pa.large_string()))
        self.all_ref = np.concatenate(self.ref_code) if self.ref_code else np.zeros(0, np.int32)
        self.all_rg = np.concatenate(self.rg_code) if self.rg_code else np.zeros(0, np.int32)


def fold_codes(codes: Sequence[int], values: list, numeric: bool):
    """PileupAggregator's pairwise fold of one recordGroup field over the rows
    of a group, given as codes into `values`"""
    v = values[codes[0]]
    for c in codes[1:]:
        w = values[c]
        if numeric:
            d = {x for x in (v, w) if x is not None}
            v = d.pop() if len(d) == 1 else None
        elif v is None or w is None or v == w:
            v = w if v is None else v
        else:
            v = v + "," + w
    return v


def group_table(F: Dict[str, np.ndarray], U: Units, g0: int, g1: int):
    """The ADAMPileup table of groups [g0, g1) of a fetched result."""
    import pyarrow as pa
    import pyarrow.compute as pc
    n = g1 - g0
    if n <= 0:
        return pileup_schema().empty_table()
    pb = pa.py_buffer
    G = len(F["first_row"])

    def ints(name, typ, valid=None):
        return pa.Array.from_buffers(typ, G, [pb(F[valid]) if valid else None, pb(F[name])]).slice(g0, n)

    def base(name):
        ind = pa.Array.from_buffers(pa.int8(), G, [pb(F[name + "_valid"]), pb(F[name])]).slice(g0, n)
        return pa.DictionaryArray.from_arrays(ind, pa.array(BASES, pa.string()), safe=False)

    cols = {
        "referenceId": ints("reference_id", pa.int32()),
        "position": ints("position", pa.int64()),
        "rangeOffset": ints("range_offset", pa.int32(), "range_offset_valid"),
        "rangeLength": ints("range_length", pa.int32(), "range_length_valid"),
        "referenceBase": base("reference_base"),
        "readBase": base("read_base"),
        "sangerQuality": ints("sanger_quality", pa.int32()),
        "mapQuality": ints("map_quality", pa.int32()),
        "numSoftClipped": ints("num_soft_clipped", pa.int32(), "num_soft_clipped_valid"),
        "numReverseStrand": ints("num_reverse_strand", pa.int32(), "num_reverse_strand_valid"),
        "countAtPosition": ints("count_at_position", pa.int32()),
        "readStart": ints("read_start", pa.int64(), "read_start_valid"),
        "readEnd": ints("read_end", pa.int64(), "read_end_valid"),
    }
    off = F["offsets"][g0:g1 + 1].astype(np.int64)
    units = F["names"][off[0]:off[-1]]  # the units of the groups' rows, in fold order
    rel = off - off[0]
    first = units[rel[:-1]]
    lone = np.diff(rel) == 1
    # readName: a + "," + b over the group; a null name prints as "null" unless the row is alone
    names = U.all_names.take(pa.array(units, pa.int32()))
    null_alone = None
    if names.null_count:
        null_alone = lone & ~np.asarray(names.take(pa.array(rel[:-1])).is_valid().to_numpy(zero_copy_only=False), bool)
        names = names.fill_null("null")
    lists = pa.LargeListArray.from_arrays(pa.array(rel, pa.int64()), names)
    joined = pc.binary_join(lists, pa.scalar(",", pa.large_string())).cast(pa.string())
    if null_alone is not None and null_alone.any():
        joined = pc.if_else(pa.array(null_alone), pa.scalar(None, pa.string()), joined)
    cols["readName"] = joined
    # referenceName: the first row's
    rc = U.all_ref[first]
    ok = rc >= 0
    dic = pa.array([v if v is not None else "" for v in (U.ref_values or [None])], pa.string())
    cols["referenceName"] = pa.DictionaryArray.from_arrays(
        pa.array(np.where(ok, rc, 0).astype(np.int32), mask=None if ok.all() else ~ok), dic, safe=False)
    # the recordGroup fields are dictionary arrays: a group whose rows share one code takes that
    # code's value; the others (several libraries of one sample at a position) take the fold of
    # their code sequence, folded once per distinct sequence (found per group length by
    # numpy.unique over the rows' codes) and appended to the dictionary.  Python work is per
    # distinct sequence: slow where deep groups rarely repeat one.
    w0 = g0 // 64  # (only this part's words: unpacking the whole bitmap for every part is quadratic)
    uniform = np.unpackbits(F["uniform_rg"][w0:(g1 + 63) // 64].view(np.uint8),
                            bitorder="little")[g0 - w0 * 64:g1 - w0 * 64].astype(bool)
    code = U.all_rg[first].astype(np.int64)
    mixed = np.flatnonzero(~uniform)
    seqs: List[tuple] = []
    seq_id = np.zeros(len(mixed), np.int64)
    if len(mixed):
        rg_rows = U.all_rg[units]
        lens = rel[mixed + 1] - rel[mixed]
        bits = max(1, int(rg_rows.max()).bit_length())
        for length in np.unique(lens):
            sel = np.flatnonzero(lens == length)
            mat = rg_rows[rel[mixed[sel]][:, None] + np.arange(length)]
            if length * bits <= 62:  # the sequence as one integer: a plain sort finds the distinct ones
                packed = (mat.astype(np.int64) << (bits * np.arange(length, dtype=np.int64))).sum(axis=1)
                _, at, inv = np.unique(packed, return_index=True, return_inverse=True)
                uniq = mat[at]
            else:
                uniq, inv = np.unique(mat, axis=0, return_inverse=True)
            seq_id[sel] = len(seqs) + inv.reshape(-1)
            seqs.extend(tuple(int(c) for c in r) for r in uniq)
    t = {"string": pa.string(), "int32": pa.int32(), "int64": pa.int64()}
    kinds = dict(PILEUP_FIELDS)
    for f in RG_FIELDS:
        values = list(U.rg_values[f]) + [fold_codes(q, U.rg_values[f], f in RG_NUMBER) for q in seqs]
        typ = t[kinds[f]]
        has = np.array([v is not None for v in values], bool)
        if not has.any():
            cols[f] = pa.nulls(n, typ)
            continue
        idx = code.copy()
        idx[mixed] = len(U.rg_values[f]) + seq_id
        ok = has[idx]
        dic = pa.array([v if v is not None else ("" if kinds[f] == "string" else 0) for v in values], typ)
        cols[f] = pa.DictionaryArray.from_arrays(
            pa.array(np.where(ok, idx, 0).astype(np.int32), mask=None if ok.all() else ~ok), dic, safe=False)
    return pa.table([cols[name] for name, _ in PILEUP_FIELDS], names=[name for name, _ in PILEUP_FIELDS])


def _flat(col, typ):
    """a table column as one Arrow array of type typ with offset 0"""
    import pyarrow as pa
    c = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    if isinstance(c, pa.ChunkedArray):
        c = pa.concat_arrays(c.chunks) if c.num_chunks else pa.nulls(0, typ)
    if c.type != typ:
        c = c.cast(typ)
    if c.offset:
        c = pa.concat_arrays([c])
    return c


def _dict_codes(col):
    """(codes with -1 for null, values) of a string / integer column"""
    import pyarrow as pa
    import pyarrow.compute as pc
    c = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    if isinstance(c, pa.ChunkedArray):
        c = pa.concat_arrays(c.chunks) if c.num_chunks else pa.nulls(0, col.type)
    if pa.types.is_dictionary(c.type):
        c = c.cast(c.type.value_type)
    d = c.dictionary_encode()
    codes = np.asarray(pc.fill_null(d.indices, -1).to_numpy(zero_copy_only=False), np.int64)
    return codes, d.dictionary.to_pylist()


def table_units(table, U: Units):
    """The units of an Arrow table of ADAMPileup rows or ADAMRecords: its
    readName and referenceName columns, and one record-group code per
    distinct tuple of the ten recordGroup columns.  Returns (rg_code,
    sample_code) per row of the table."""
    import pyarrow as pa
    n = table.num_rows
    have = set(table.column_names)
    names = _flat(table.column("readName"), pa.string()) if "readName" in have else pa.nulls(n, pa.string())
    if "referenceName" in have:
        ref_code, U.ref_values = _dict_codes(table.column("referenceName"))
    else:
        ref_code, U.ref_values = np.full(n, -1, np.int64), []
    per_field = {}
    key = np.zeros(n, np.int64)
    radix = 1
    wide = False
    for f in RG_FIELDS:
        codes, values = _dict_codes(table.column(f)) if f in have else (np.full(n, -1, np.int64), [])
        per_field[f] = (codes, values)
        if radix * (len(values) + 1) >= 1 << 62:
            wide = True
        else:
            key += (codes + 1) * radix
            radix *= len(values) + 1
    if wide:  # (more distinct tuples than one int64 numbers: the slow way)
        mat = np.stack([per_field[f][0] for f in RG_FIELDS], axis=1)
        _, firsts, inverse = np.unique(mat, axis=0, return_index=True, return_inverse=True)
    else:
        _, firsts, inverse = np.unique(key, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    for f in RG_FIELDS:
        codes, values = per_field[f]
        U.rg_values[f] = [None if codes[i] < 0 else values[codes[i]] for i in firsts] or [None]
    rg_code = inverse.astype(np.int32)
    ranks = sample_ranks(U.rg_values["recordGroupSample"])
    U.add(names, ref_code, rg_code)
    return rg_code, (ranks[rg_code] if n else np.zeros(0, np.int32))


def add_pileup_table(agg: Aggregation, table, U: Units, add_rows: int = _ADD_ROWS):
    """ADAMPileup rows of an Arrow table into the aggregation, add_rows rows per add"""
    import pyarrow as pa
    import pyarrow.compute as pc
    rg_code, sample_code = table_units(table, U)
    have = set(table.column_names)
    bases = pa.array(BASES, pa.string())
    for a in range(0, table.num_rows, max(1, add_rows)):
        sl = table.slice(a, max(1, add_rows))
        m = sl.num_rows
        cols, valid = {}, {}
        for f, name, dt in _ROWS:
            if name is None or name not in have:
                continue
            if dt == np.uint8:
                src = _flat(sl.column(name), pa.string())
                c = pc.index_in(src, value_set=bases)
                if c.null_count != src.null_count:
                    raise ValueError("%s holds a value outside the Base enum" % name)
                c = _flat(c.cast(pa.uint8()), pa.uint8())
            else:
                c = _flat(sl.column(name), pa.int64() if dt == np.int64 else pa.int32())
            b = c.buffers()
            cols[f] = np.frombuffer(b[1], dt, m) if m else np.zeros(0, dt)
            if b[0] is not None and c.null_count:
                valid[f] = np.frombuffer(b[0], np.uint8, (m + 7) // 8)
        sm = sample_code[a:a + m]
        cols["sample_code"] = np.where(sm >= 0, sm, 0).astype(np.int32)
        if (sm < 0).any():
            valid["sample_code"] = np.packbits(sm >= 0, bitorder="little")
        cols["rg_code"] = rg_code[a:a + m]
        agg.add_host(m, cols, valid)


def _sam_units(U: Units, hdr):
    """the header's record groups as codes (0: no record group, 1 + recordGroupId
    otherwise) and references; the sample rank of every code"""
    U.ref_values = [r["SN"] for r in hdr.sq]
    U.rg_values["recordGroupRunDateEpoch"] = [None] + hdr.rg_column("DT", "date")
    U.rg_values["recordGroupPredictedMedianInsertSize"] = [None] + hdr.rg_column("PI", "int")
    for name, key in RG_TAGS:
        U.rg_values[name] = [None] + hdr.rg_column(key)
    return sample_ranks(U.rg_values["recordGroupSample"])


def aggregate_pileups(inp: str, out: str, compression: str = "gzip", part_rows: int = DEFAULT_PART_ROWS,
                      partition_bytes: Optional[int] = None, overwrite: bool = False, device: int = 0,
                      part_reads: int = R.DEFAULT_PART_READS, writer_args: Optional[dict] = None,
                      region: Optional[str] = None, bai: Optional[str] = None) -> Dict[str, object]:
    """`adam aggregate_pileups`: the ADAMPileup rows of `inp` (ADAMPileup
    Parquet; or SAM, BAM or ADAMRecord Parquet, expanded as reads2ref does)
    aggregated by position into ADAMPileup Parquet part files under `out`,
    which appears only when the job succeeds.  part_rows: aggregated rows per
    part file; partition_bytes: SAM text per streamed partition; part_reads:
    reads per expansion call.  region, bai: BAM input read through its .bai index, only the reads that overlap the region (inputs.SamInput).  Returns the job's statistics."""
    from . import parquet as P
    region = region_plan(inp, region, bai)  # (refused before anything is read or created)
    partition_bytes = DEFAULT_PARTITION_BYTES if partition_bytes is None else partition_bytes
    check_out(out, overwrite, True)
    ctx = bqsr.Context.get(device)
    ph = Phases()
    part_rows, part_reads = max(1, int(part_rows)), max(1, int(part_reads))
    stats: Dict[str, object] = {}
    U = Units()
    L = R._lib()
    with Aggregation(ctx) as agg:
        if is_parquet(inp):
            import pyarrow.parquet as pq
            schema_names = set(pq.ParquetDataset(inp).schema.names)
            if "countAtPosition" in schema_names or "readBase" in schema_names:  # ADAMPileup rows
                with ph("read"):
                    table = P.read_table(inp, [n for n, _ in PILEUP_FIELDS])
                with ph("add"):
                    add_pileup_table(agg, table, U)
                stats["input"] = "pileups"
            else:
                with ph("read"):
                    table = R.locus_filter(P.read_table(inp, R.PROJECTION))
                if "referenceId" not in table.column_names:  # (every referenceId null: the rows throw, as they must)
                    import pyarrow as pa
                    table = table.append_column("referenceId", pa.nulls(table.num_rows, pa.int32()))
                with ph("parse"):
                    A = P.ArrowReads(table, ctx, markdup=True)  # (referenceId travels with MarkDuplicates' columns)
                try:
                    with ph("add"):
                        rg_code, sample_code = table_units(table, U)
                        for r0 in range(0, table.num_rows, part_reads):
                            m = min(part_reads, table.num_rows - r0)
                            sz = R._arrow_prepare(A, r0, m)
                            agg.add_arrow(A, sz.n_rows, sample_code[r0:r0 + m], rg_code[r0:r0 + m], r0)
                finally:
                    A.close()
                stats["input"] = "reads"
                stats["reads"] = table.num_rows
        else:
            n_reads = 0
            with SamInput(inp, ctx, ph, partition_bytes, region=region, bai=bai) as src:
                for sam, base in src:
                    stats.update(src.region_stats or {})
                    hdr = header_info(sam)
                    ranks = _sam_units(U, hdr)
                    n = sam.counts().n_reads
                    with ph("add"):
                        for r0 in range(0, n, part_reads):
                            m = min(part_reads, n - r0)
                            sz = R.PileupSizes()
                            try:
                                check(L.bqsr_sam_pileup_prepare(ctx.handle, sam.h, r0, m, None, ctypes.byref(sz)))
                            except _capi.BQSRError as e:
                                raise rebased(e, base) from None
                            rl = R._sam_read_level(sam, r0, m, hdr)
                            ref, ref_ok, _ = rl.coded["referenceId"]
                            rg, rg_ok, _ = rl.coded["recordGroupSample"]
                            code = np.where(rg_ok, rg + 1, 0).astype(np.int32)
                            agg.add_sam(sam, sz.n_rows, ranks[code], code, base + r0)
                            U.add(rl.read_name, np.where(ref_ok, ref, -1), code)
                    n_reads = base + n
            stats["input"] = "reads"
            stats["reads"] = n_reads
        with ph("aggregate"):
            sz = agg.run()
        stats["kernel_ms"] = kernel_times()
        with ph("fetch"):
            F = agg.fetch(sz)
    stats["rows_in"], stats["rows_out"] = int(sz.n_rows), int(sz.n_groups)
    U.freeze()
    W = AdamWriter(out, compression, overwrite=overwrite, dict_cols=PILEUP_DICT_COLS, stats_cols=PILEUP_STATS_COLS,
                   huffman_cols=(), max_pending=2, **(writer_args or {}))
    ok = False
    try:
        # the parts' tables are built a few ahead by host threads (Arrow and numpy release the
        # interpreter lock) and handed to the writer in order
        import collections
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(_TABLE_THREADS) as pool:
            ahead = collections.deque()
            starts = iter(range(0, sz.n_groups, part_rows))
            while True:
                while len(ahead) < 2 * _TABLE_THREADS:
                    g0 = next(starts, None)
                    if g0 is None:
                        break
                    ahead.append(pool.submit(group_table, F, U, g0, min(sz.n_groups, g0 + part_rows)))
                if not ahead:
                    break
                with ph("strings"):
                    t = ahead.popleft().result()
                with ph("write"):
                    W.add(t)
        if W.parts == 0:  # no rows at all: one empty part file carries the schema
            W.add(pileup_schema().empty_table())
        ok = True
    finally:
        with ph("close"):
            W.close(ok)
    stats["parts"] = W.parts
    stats["phases"] = ph.t
    return stats


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="adam_amd.aggregate_pileups", description=__doc__.split("\n\n")[0])
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("-parquet_compression", default="gzip", choices=("gzip", "snappy", "none"))
    ap.add_argument("-part_rows", type=int, default=DEFAULT_PART_ROWS, help="aggregated rows per part file")
    ap.add_argument("-partition_bytes", type=int, default=DEFAULT_PARTITION_BYTES,
                    help="SAM text per streamed partition, in bytes")
    ap.add_argument("-overwrite", action="store_true")
    add_region_arguments(ap)
    a = ap.parse_args(argv)
    try:
        a.region = region_plan(a.input, a.region, a.bai)
    except (ValueError, OSError) as e:
        ap.error(str(e))
    t0 = time.perf_counter()
    st = aggregate_pileups(a.input, a.output, a.parquet_compression, a.part_rows, a.partition_bytes, a.overwrite,
                           region=a.region, bai=a.bai)
    report(st, t0)
    return 0


if __name__ == "__main__":
    sys.exit(main())
