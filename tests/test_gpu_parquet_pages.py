"""Parquet data pages built on the device (adam_amd/csrc/parquet_pages.hip)
against the numpy restatement of the page forms (tests/_parquet_pages_ref.py),
byte for byte, with 128-row pages; then `reads2ref -parquet_encoder device` end
to end: its files read back equal to the host path's on the same input."""
import functools
import glob
import os

import numpy as np
import pytest

import _parquet_pages_ref as R
import _pileup_gen as G
from adam_amd import _capi, adam_save, bam_writer, bqsr, reads2ref
from adam_amd import parquet_pages as PP

pytestmark = pytest.mark.gpu

PAGE_ROWS = 128
ROW_COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 300)
WIDTHS = (1, 5, 8, 9, 17, 32)
RES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_resources")


@pytest.fixture(scope="module")
def enc():
    e = PP.Encoder(bqsr.Context.get(0))
    yield e
    e.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def check(enc, kind, src, n, w=0, gather=None, remap=None, base=0, validity=None, page_rows=PAGE_ROWS):
    """encode on the device, compare bodies and page table with the restatement; returns the Stream"""
    src = np.asarray(src)
    held = [dev(src if len(src) else np.zeros(1, src.dtype))]
    col = PP.ParquetColumn(kind=kind, src_width=src.dtype.itemsize, src=held[0].data_ptr(), src_n=len(src),
                           bit_width=w, base=base)
    if gather is not None:
        held.append(dev(np.asarray(gather, np.int32)))
        col.gather = held[-1].data_ptr()
    if remap is not None:
        held.append(dev(np.asarray(remap, np.int32)))
        col.remap, col.remap_n = held[-1].data_ptr(), len(remap)
    if validity is not None:
        held.append(dev(R.bitmap_words(validity).view(np.int64)))
        col.validity = held[-1].data_ptr()
    st = enc.encode(col, n, page_rows)
    values, valid = R.row_values(n, src, gather, remap, base, validity)
    bodies, pages = R.column_pages(kind, values, valid, page_rows, w)
    assert np.array_equal(st.pages, pages), (st.pages.tolist(), pages.tolist())
    assert bytes(st.bodies) == bodies
    return st


def patterns(n):
    i = np.arange(n)
    p = {"valid": np.ones(n, bool), "null": np.zeros(n, bool), "alternating": i % 2 == 0,
         "word_straddle": ~((i >= 57) & (i < 71)), "page_straddle": ~((i >= 120) & (i < 141)),
         "sparse": i % 37 == 5}
    return p


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_counts_and_validity_patterns(enc, n):
    rng = np.random.default_rng(n)
    codes = rng.integers(0, 17, n).astype(np.uint8)
    i32 = rng.integers(-1 << 31, 1 << 31, n).astype(np.int32)
    i64 = rng.integers(-1 << 63, 1 << 63, n, dtype=np.int64)
    for name, valid in patterns(n).items():
        validity = None if name == "valid" else valid
        check(enc, PP.DICT_INDEX, codes, n, 5, validity=validity)
        check(enc, PP.PLAIN_INT32, i32, n, validity=validity)
        check(enc, PP.PLAIN_INT64, i64, n, validity=validity)


@pytest.mark.parametrize("non_nulls", (8, 64, 128))
def test_exact_non_null_counts(enc, non_nulls):
    n = 300
    rng = np.random.default_rng(non_nulls)
    for first_page_only in (True, False):  # all within one page, or spread over the three
        valid = np.zeros(n, bool)
        valid[rng.choice(PAGE_ROWS if first_page_only else n, non_nulls, replace=False)] = True
        assert valid.sum() == non_nulls
        check(enc, PP.DICT_INDEX, rng.integers(0, 500, n).astype(np.int32), n, 9, validity=valid)
        check(enc, PP.PLAIN_INT64, rng.integers(0, 1 << 40, n), n, validity=valid)
    valid = np.ones(PAGE_ROWS, bool)  # a page of exactly 128 non-nulls: two full blocks, no tail
    check(enc, PP.DICT_INDEX, rng.integers(0, 500, PAGE_ROWS).astype(np.int32), PAGE_ROWS, 9, validity=valid)


def test_block_rule(enc):
    # page 0: an equal block, then the same again (two RLE runs, not merged); page 1: an equal block, then a
    # different equal one; page 2: an equal block, then one equal but for its last lane (bit-packed); page 3:
    # a mixed block, then an equal one; page 4: a tail of 5 values
    v = np.concatenate([np.full(64, 7), np.full(64, 7), np.full(64, 7), np.full(64, 3), np.full(64, 5),
                        np.r_[np.full(63, 5), 4], np.arange(64) % 8, np.full(64, 0), [1, 2, 3, 4, 5]]).astype(np.int32)
    st = check(enc, PP.DICT_INDEX, v, len(v), 3)
    sizes = st.pages[:, 1].tolist()
    lev = 4 + 1 + 16  # length, run header, 128 bits
    rle, packed = 2 + 1, 1 + 8 * 3
    assert sizes == [lev + 1 + rle + rle, lev + 1 + rle + rle, lev + 1 + rle + packed, lev + 1 + packed + rle,
                     4 + 1 + 1 + 1 + 1 + 3]
    # the same values behind nulls: blocks are cut from the NON-NULL values, across row words
    valid = np.arange(2 * len(v)) % 2 == 1
    check(enc, PP.DICT_INDEX, np.repeat(v, 2), 2 * len(v), 3, validity=valid)
    # larger pages: more blocks per page, and a tail of 1, 7 and 8 values
    for tail in (1, 7, 8):
        w = np.r_[v[:448], np.arange(tail)].astype(np.int32)
        check(enc, PP.DICT_INDEX, w, len(w), 3, page_rows=256)
        check(enc, PP.DICT_INDEX, w, len(w), 3, page_rows=64)


@pytest.mark.parametrize("w", WIDTHS)
def test_every_width(enc, w):
    rng = np.random.default_rng(w)
    n = 300
    v = rng.integers(0, 1 << w, n).astype(np.uint32).view(np.int32)
    v[:3] = np.array([(1 << w) - 1, 0, 1 << (w - 1)], np.uint32).view(np.int32)  # every bit of the width
    v[128:192] = v[128]  # an RLE run of a wide value
    if w <= 8:
        check(enc, PP.DICT_INDEX, v.astype(np.uint8), n, w)
    # int32 sources: at width 32 the top bit makes the source negative; only the low w bits are written
    check(enc, PP.DICT_INDEX, v, n, w, validity=np.arange(n) % 3 != 0)
    check(enc, PP.DICT_INDEX, v, n, w)


def test_gather_and_remap(enc):
    rng = np.random.default_rng(7)
    reads = 23
    codes = rng.integers(0, 6, reads).astype(np.int32)
    codes[[2, 9]] = -1   # reads whose field is null
    codes[11] = 6        # a code beyond the table: null
    read = np.sort(rng.integers(0, reads, 300)).astype(np.int32)
    remap = np.array([0, -1, 2, 3, -1, 5], np.int32)  # entries without a value: -1
    st = check(enc, PP.DICT_INDEX, codes, 300, 3, gather=read, remap=remap)
    assert 0 < st.pages[:, 3].sum() < 300
    check(enc, PP.DICT_INDEX, codes, 300, 3, gather=read, remap=remap, validity=np.arange(300) % 5 != 0)
    check(enc, PP.DICT_INDEX, codes, 300, 3, gather=read, remap=np.full(6, -1, np.int32))  # every row null
    check(enc, PP.DICT_INDEX, codes, 300, 3, gather=read, remap=np.array([-1], np.int32))
    # a remap without gather (readName's nulls), a gather without remap, a gather of PLAIN values
    check(enc, PP.DICT_INDEX, read, 300, 5, remap=np.where(np.arange(reads) % 4, np.arange(reads), -1))
    check(enc, PP.DICT_INDEX, np.abs(codes), 300, 3, gather=read)
    check(enc, PP.PLAIN_INT64, rng.integers(-1 << 50, 1 << 50, reads), 300, gather=read)
    # a table of zeros turns any byte column into the constant index 0 (countAtPosition)
    st = check(enc, PP.DICT_INDEX, rng.integers(0, 17, 300).astype(np.uint8), 300, 1, remap=np.zeros(256, np.int32))
    assert st.pages[:, 1].tolist() == [4 + 1 + 16 + 1 + 3 + 3, 4 + 1 + 16 + 1 + 3 + 3, 4 + 1 + 6 + 1 + 1 + 6]


def plain_desc(held, src, n, validity=None):
    held.append(dev(src))
    col = PP.ParquetColumn(kind=PP.PLAIN_INT32, src_width=4, src=held[-1].data_ptr(), src_n=len(src))
    if validity is not None:
        held.append(dev(R.bitmap_words(validity).view(np.int64)))
        col.validity = held[-1].data_ptr()
    return col


def test_dense_range_and_its_fallback(enc):
    rng = np.random.default_rng(3)
    n = 300
    valid = rng.random(n) > 0.2
    held = []
    # a narrow range becomes a dictionary [min, max] over the NON-NULL values, index = value - min
    v = rng.integers(-5, 40, n).astype(np.int32)
    v[~valid] = 100000  # (null slots do not widen the range)
    lo, hi = int(v[valid].min()), int(v[valid].max())
    col = plain_desc(held, v, n, valid)
    assert enc.minmax(col, n) == (lo, hi, int(valid.sum()))
    c = PP.small_int_column(enc, "x", col, n, PAGE_ROWS)
    assert c.dictionary == PP.plain_ints(np.arange(lo, hi + 1), "int32")
    w = PP.bit_width(hi - lo + 1)
    bodies, pages = R.column_pages(R.DICT_INDEX, np.where(valid, v - lo, 0), valid, PAGE_ROWS, w)
    assert bytes(c.stream.bodies) == bodies and np.array_equal(c.stream.pages, pages)
    # exactly 65536 entries: still a dictionary, at width 16; one more: PLAIN
    for span, dictionary in ((65535, True), (65536, False)):
        v = rng.integers(1000, 1000 + span + 1, n).astype(np.int32)
        v[[5, 250]] = 1000, 1000 + span
        c = PP.small_int_column(enc, "x", plain_desc(held, v, n), n, PAGE_ROWS)
        if dictionary:
            assert c.dictionary[1] == 65536
            want = R.column_pages(R.DICT_INDEX, v - 1000, np.ones(n, bool), PAGE_ROWS, 16)
        else:
            assert c.dictionary is None
            want = R.column_pages(R.PLAIN_INT32, v, np.ones(n, bool), PAGE_ROWS)
        assert bytes(c.stream.bodies) == want[0] and np.array_equal(c.stream.pages, want[1])
    # no value at all: a one-entry dictionary nothing points into
    c = PP.small_int_column(enc, "x", plain_desc(held, v, n, np.zeros(n, bool)), n, PAGE_ROWS)
    assert c.dictionary == PP.plain_ints([0], "int32") and c.stream.pages[:, 3].sum() == 0
    assert enc.minmax(plain_desc(held, v, n, np.zeros(n, bool)), n)[2] == 0


def test_many_pages_and_grid_stride(enc):
    """more items than one pass of a capped grid takes, every kind"""
    rng = np.random.default_rng(11)
    n = 20000
    valid = rng.random(n) > 0.3
    v = (rng.integers(0, 1 << 17, n) * (rng.random(n) > 0.5)).astype(np.int32)  # zero runs: some RLE blocks
    v[4096:8192] = 77
    ctx = bqsr.Context.get(0)
    for g in (0, 1, 3):
        with ctx.tuned(pileup_grid=g):
            check(enc, PP.DICT_INDEX, v, n, 17, validity=valid)
            check(enc, PP.PLAIN_INT32, v, n, validity=valid)
            check(enc, PP.DICT_INDEX, v, n, 17, page_rows=4096)
    size_ms, emit_ms = PP.kernel_times()
    assert size_ms > 0.0 and emit_ms > 0.0


def test_refusals(enc):
    held = []
    col = plain_desc(held, np.arange(64, dtype=np.int32), 64)
    with pytest.raises(_capi.BQSRError) as e:
        enc.encode(col, 64, 100)
    assert e.value.name == "INVALID_ARG"
    with pytest.raises(_capi.BQSRError):
        enc.encode(col, 65, PAGE_ROWS)  # the source does not cover the rows
    with pytest.raises(_capi.BQSRError):
        _capi.check(PP._lib().bqsr_parquet_pages_emit(enc.h, None, None, None))  # no size call before it


# ---- end to end ------------------------------------------------------------------

E = (0, "nomd"), (5, "star"), (0, "skips")


def read_output(path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    parts = sorted(glob.glob(os.path.join(path, "part-r-*.parquet")))
    assert parts and os.path.exists(os.path.join(path, "_SUCCESS"))
    assert not os.path.lexists(path + ".partial")
    return pa.concat_tables([pq.read_table(p) for p in parts]), len(parts)


@functools.lru_cache(maxsize=None)
def e2e_text():
    # reads without rows at part edges (part_reads 64: reads 63, 64, 127, 128 ...), two read groups
    specs = tuple(E[i % 3] if i % 64 in (0, 63) or i % 6 == 0 else (25 + i % 40, None) for i in range(400))
    return G.generated(specs, 21, True)[0]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """the generated reads as SAM, BAM and ADAM Parquet, and each input's host-path output (computed once)"""
    from adam_amd.transform import transform
    d = tmp_path_factory.mktemp("pages_e2e")
    text = e2e_text()
    paths = {k: str(d / ("in." + k)) for k in ("sam", "bam", "adam")}
    open(paths["sam"], "wb").write(text)
    open(paths["bam"], "wb").write(bam_writer.sam_to_bam(text))
    transform(paths["sam"], paths["adam"], part_reads=256)
    host = {}
    for k, p in paths.items():
        out = str(d / ("host_" + k + ".adam"))
        reads2ref.reads2ref(p, out, part_reads=64, compression="snappy")
        host[k] = read_output(out)
    return paths, host


@pytest.mark.parametrize("codec", ["gzip", "snappy", "none"])
@pytest.mark.parametrize("kind", ["sam", "bam", "adam"])
def test_reads2ref_device_pages_equal_the_host_path(inputs, tmp_path, kind, codec):
    import pyarrow.parquet as pq
    paths, host = inputs
    out = str(tmp_path / "dev.adam")
    st = reads2ref.reads2ref(paths[kind], out, part_reads=64, compression=codec, parquet_encoder="device",
                             page_rows=PAGE_ROWS)
    got, parts = read_output(out)
    want, want_parts = host[kind]
    assert want.num_rows > 5000 and parts == want_parts == st["parts"] and parts > 3
    assert got.schema.equals(want.schema) and got.schema.equals(adam_save.pileup_schema())
    assert got.equals(want)  # values and nulls
    assert st["pileups"] == want.num_rows and st["page_bytes_downloaded"] > 0
    assert st["file_bytes"] == sum(os.path.getsize(p) for p in glob.glob(os.path.join(out, "part-r-*")))
    first = os.path.join(out, "part-r-00000.parquet")
    md, t = pq.ParquetFile(first).metadata.row_group(0), pq.read_table(first)
    assert md.column(2).compression == {"gzip": "GZIP", "snappy": "SNAPPY", "none": "UNCOMPRESSED"}[codec]
    for i in range(t.num_columns):  # the footer's null counts are the table's
        assert md.column(i).statistics.null_count == t.column(i).null_count, t.column_names[i]


@pytest.mark.parametrize("kind", ["sam", "adam"])
def test_read_spans_as_plain_int64(inputs, tmp_path, monkeypatch, kind):
    """readStart / readEnd as the per-read dictionary and as PLAIN int64 (READ_SPANS picks by codec): one table"""
    import pyarrow.parquet as pq
    paths, host = inputs
    sizes = {}
    for form in ("dictionary", "plain"):
        monkeypatch.setattr(reads2ref, "READ_SPANS", dict.fromkeys(reads2ref.READ_SPANS, form))
        out = str(tmp_path / (form + ".adam"))
        reads2ref.reads2ref(paths[kind], out, part_reads=64, compression="none", parquet_encoder="device",
                            page_rows=PAGE_ROWS)
        assert read_output(out)[0].equals(host[kind][0])
        rg = pq.ParquetFile(os.path.join(out, "part-r-00000.parquet")).metadata.row_group(0)
        sizes[form] = rg.column(13).has_dictionary_page, rg.column(13).total_uncompressed_size
    assert sizes["dictionary"][0] and not sizes["plain"][0] and sizes["dictionary"][1] < sizes["plain"][1]


@pytest.mark.parametrize("name", ["artificial.sam", "artificial.realigned.sam", "small_realignment_targets.sam"])
def test_golden_fixtures(tmp_path, name):
    host, dev_out = str(tmp_path / "host.adam"), str(tmp_path / "dev.adam")
    src = os.path.join(RES, name)
    reads2ref.reads2ref(src, host, part_reads=3)
    # (the command line, default page size)
    assert reads2ref.main([src, dev_out, "-part_reads", "3", "-parquet_encoder", "device"]) == 0
    got, want = read_output(dev_out), read_output(host)
    assert got[1] == want[1] and want[0].num_rows > 0
    assert got[0].schema.equals(want[0].schema) and got[0].equals(want[0])


def test_no_reads_and_overwrite(tmp_path):
    import pyarrow.parquet as pq
    inp, host, out = str(tmp_path / "in.sam"), str(tmp_path / "host.adam"), str(tmp_path / "dev.adam")
    open(inp, "wb").write(G.HEADER)
    reads2ref.reads2ref(inp, host)
    st = reads2ref.reads2ref(inp, out, parquet_encoder="device")
    assert st["parts"] == 1 and st["pileups"] == 0
    got, want = read_output(out), read_output(host)
    assert got[1] == want[1] == 1 and got[0].num_rows == 0 and got[0].equals(want[0])
    a = pq.ParquetFile(os.path.join(out, "part-r-00000.parquet"))
    b = pq.ParquetFile(os.path.join(host, "part-r-00000.parquet"))
    assert a.schema.equals(b.schema)
    with pytest.raises(FileExistsError):
        reads2ref.reads2ref(inp, out, parquet_encoder="device")
    reads2ref.reads2ref(inp, out, parquet_encoder="device", overwrite=True)
    assert read_output(out)[0].num_rows == 0
    with pytest.raises(ValueError):
        reads2ref.reads2ref(inp, str(tmp_path / "x.adam"), parquet_encoder="elsewhere")
    assert not os.path.lexists(str(tmp_path / "x.adam"))


def test_a_throwing_read_leaves_no_output(tmp_path):
    text = e2e_text()
    lines = text[len(G.HEADER):].splitlines(True)
    lines[333] = b"\t".join([b"bad", b"16", b"c1", b"101", b"30", b"2M", b"*", b"0", b"0", b"Ac", b"II",
                             b"MD:Z:2"]) + b"\n"  # a lower-case base: Base.valueOf throws
    bad, gone = str(tmp_path / "bad.sam"), str(tmp_path / "gone.adam")
    open(bad, "wb").write(G.HEADER + b"".join(lines))
    with pytest.raises(_capi.BQSRError) as e:
        reads2ref.reads2ref(bad, gone, partition_bytes=len(text) // 4, part_reads=64, parquet_encoder="device",
                            page_rows=PAGE_ROWS)
    assert (e.value.name, e.value.read) == ("PILEUP", 333)
    assert not os.path.lexists(gone) and not os.path.lexists(gone + ".partial")
