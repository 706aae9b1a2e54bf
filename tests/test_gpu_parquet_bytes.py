"""PLAIN BYTE_ARRAY and PLAIN BOOLEAN data pages built on the device
(adam_amd/csrc/parquet_pages.hip: bqsr_parquet_pages_size_strings / _bools)
against the numpy restatement (tests/_parquet_bytes_ref.py), byte for byte,
with 128-row pages; then `transform -parquet_encoder device` end to end: its
part files read back equal to the host path's for the same call."""
import functools
import glob
import os

import numpy as np
import pytest

import _parquet_bytes_ref as B
import _parquet_pages_ref as R
from adam_amd import _capi, adam_pages, adam_save, bqsr, synth
from adam_amd import parquet_pages as PP
from adam_amd.bam_writer import sam_to_bam
from adam_amd.samgen import sam_text
from adam_amd.transform import main as transform_main, transform
from test_gpu_adam_out import FIXTURES, GOLD
from test_gpu_parquet_pages import dev, patterns, read_output

pytestmark = pytest.mark.gpu

PAGE_ROWS = 128
ROW_COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 300)
LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257)
PREAMBLE_128 = 4 + 1 + 16  # of a full page: length, run header, 128 bits


@pytest.fixture(scope="module")
def enc():
    e = PP.Encoder(bqsr.Context.get(0))
    yield e
    e.close()


def words(bits, n_fill=None):
    """an Arrow bitmap's u64 words on the device; n_fill: the last word's bits from row n_fill on set"""
    w = R.bitmap_words(bits).copy()
    if n_fill is not None and n_fill % 64:
        w[n_fill // 64] |= np.uint64(~((1 << (n_fill % 64)) - 1) & 0xFFFFFFFFFFFFFFFF)
    return dev(w.view(np.int64))


def check_strings(enc, strings, valid=None, page_rows=PAGE_ROWS, want=None):
    """strings: bytes objects, every row's (a null row keeps its bytes in the source); valid: None for no bitmap;
    want: the restatement's (bodies, pages) when the caller has them already.  Returns the Stream and `want`."""
    off, data, _ = B.arrow_strings(strings)
    n = len(strings)
    held = [dev(off), dev(data if len(data) else np.zeros(1, np.uint8))]
    if valid is not None:
        held.append(words(valid))
    st = adam_pages.encode_strings(enc, held[0].data_ptr(), held[1].data_ptr(),
                                   held[2].data_ptr() if valid is not None else None, n, page_rows)
    want = want or B.column_pages_strings(off, data, np.ones(n, bool) if valid is None else valid, page_rows)
    assert np.array_equal(st.pages, want[1]), (st.pages.tolist(), want[1].tolist())
    assert bytes(st.bodies) == want[0]
    return st, want


def check_bools(enc, bits, valid=None, page_rows=PAGE_ROWS, fill=True):
    """fill: the value words' bits beyond the rows are ones (they must not reach the output)"""
    n = len(bits)
    held = [words(bits, n if fill else None)]
    if valid is not None:
        held.append(words(valid))
    st = adam_pages.encode_bools(enc, held[0].data_ptr(), held[1].data_ptr() if valid is not None else None, n,
                                 page_rows)
    bodies, pages = B.column_pages_bools(bits, np.ones(n, bool) if valid is None else valid, page_rows)
    assert np.array_equal(st.pages, pages), (st.pages.tolist(), pages.tolist())
    assert bytes(st.bodies) == bodies
    return st


def random_strings(rng, n, lengths=LENGTHS):
    return [bytes(rng.integers(32, 127, k).astype(np.uint8)) for k in rng.choice(lengths, n)]


# ---- strings ----

@pytest.mark.parametrize("n", ROW_COUNTS)
def test_strings_row_counts_and_validity_patterns(enc, n):
    rng = np.random.default_rng(n)
    strings = random_strings(rng, n)  # (null rows' offsets span bytes: they must not appear)
    for name, valid in patterns(n).items():
        check_strings(enc, strings, None if name == "valid" else valid)


def test_strings_every_length(enc):
    rng = np.random.default_rng(1)
    n = 130  # three blocks over two pages
    for k in LENGTHS:
        strings = random_strings(rng, n, (k,))
        check_strings(enc, strings)
        check_strings(enc, strings, np.arange(n) % 2 == 1)
    st, _ = check_strings(enc, [b""] * n)  # only empty strings: a length word each
    assert st.pages[:, 1].tolist() == [PREAMBLE_128 + 4 * 128, 4 + 1 + 1 + 4 * 2]


def test_one_long_string_among_short_ones(enc):
    rng = np.random.default_rng(2)
    strings = random_strings(rng, 200, (0, 1, 5, 30))
    strings[77] = bytes(rng.integers(0, 256, 70_000).astype(np.uint8))
    check_strings(enc, strings)
    check_strings(enc, strings, np.arange(200) % 3 != 0)  # (row 77 stays)
    valid = np.ones(200, bool)
    valid[77] = False  # the long one null: its 70 000 bytes skipped
    st, _ = check_strings(enc, strings, valid)
    assert st.pages[:, 1].sum() < 20_000


def test_strings_all_null_page_and_exact_counts(enc):
    rng = np.random.default_rng(3)
    n = 300
    strings = random_strings(rng, n)
    valid = np.ones(n, bool)
    valid[128:256] = False  # the second page all null: its body is the preamble alone
    st, _ = check_strings(enc, strings, valid)
    assert st.pages[1].tolist()[1:] == [PREAMBLE_128, 128, 0]
    for non_nulls in (64, 128):
        for first_page_only in (True, False):
            valid = np.zeros(n, bool)
            valid[rng.choice(PAGE_ROWS if first_page_only else n, non_nulls, replace=False)] = True
            check_strings(enc, strings, valid)
    check_strings(enc, strings[:128], np.ones(128, bool))  # a page of exactly two full blocks


# ---- booleans ----

@pytest.mark.parametrize("n", ROW_COUNTS)
def test_bools_row_counts_and_validity_patterns(enc, n):
    rng = np.random.default_rng(100 + n)
    bits = rng.random(n) > 0.5
    for name, valid in patterns(n).items():
        check_bools(enc, bits, None if name == "valid" else valid)


@pytest.mark.parametrize("non_nulls", (7, 8, 9, 64, 128))
def test_bools_exact_non_null_counts(enc, non_nulls):
    n = 300
    rng = np.random.default_rng(non_nulls)
    bits = rng.random(n) > 0.5
    for first_page_only in (True, False):
        valid = np.zeros(n, bool)
        valid[rng.choice(PAGE_ROWS if first_page_only else n, non_nulls, replace=False)] = True
        st = check_bools(enc, bits, valid)
        if first_page_only:
            assert st.pages[0, 1] == PREAMBLE_128 + (non_nulls + 7) // 8
    check_bools(enc, bits[:non_nulls])  # and as a whole column without a bitmap


@pytest.mark.parametrize("n", (1, 63, 65, 127, 300))
def test_bits_beyond_the_rows_do_not_reach_the_output(enc, n):
    bits = np.zeros(n, bool)  # every value false, the rest of the last word ones: the last byte's padding stays clear
    st = check_bools(enc, bits, fill=True)
    assert not np.asarray(st.bodies)[-((n % PAGE_ROWS + 7) // 8):].any()
    # the same with a validity bitmap whose last word is ones beyond the rows
    held = [words(bits, n), words(np.ones(n, bool), n)]
    st2 = adam_pages.encode_bools(enc, held[0].data_ptr(), held[1].data_ptr(), n, PAGE_ROWS)
    assert bytes(st2.bodies) == bytes(st.bodies) and np.array_equal(st2.pages, st.pages)
    off, data, _ = B.arrow_strings([b"ab"] * n)
    held += [dev(off), dev(data)]
    st3 = adam_pages.encode_strings(enc, held[2].data_ptr(), held[3].data_ptr(), held[1].data_ptr(), n, PAGE_ROWS)
    want = B.column_pages_strings(off, data, np.ones(n, bool), PAGE_ROWS)
    assert bytes(st3.bodies) == want[0] and np.array_equal(st3.pages, want[1])


# ---- grid stride, refusals ----

def test_many_pages_and_grid_stride(enc):
    """more items than one pass of a capped grid takes, both forms"""
    rng = np.random.default_rng(11)
    n = 20000
    valid = rng.random(n) > 0.3
    strings = random_strings(rng, n, (0, 2, 7, 33, 100))
    bits = rng.random(n) > 0.5
    ctx = bqsr.Context.get(0)
    want = [None, None]  # (the restatement of the 20 000 strings once per page size)
    for g in (0, 1, 3):
        with ctx.tuned(pileup_grid=g):
            _, want[0] = check_strings(enc, strings, valid, want=want[0])
            check_bools(enc, bits, valid)
            _, want[1] = check_strings(enc, strings, None, page_rows=4096, want=want[1])
            check_bools(enc, bits, valid, page_rows=4096)
    size_ms, emit_ms = PP.kernel_times()
    assert size_ms > 0.0 and emit_ms > 0.0


def test_refusals(enc):
    off, data, _ = B.arrow_strings([b"abc"] * 64)
    held = [dev(off), dev(data), words(np.ones(64, bool))]
    with pytest.raises(_capi.BQSRError) as e:
        adam_pages.encode_strings(enc, held[0].data_ptr(), held[1].data_ptr(), None, 64, 100)
    assert e.value.name == "INVALID_ARG"
    with pytest.raises(_capi.BQSRError) as e:
        adam_pages.encode_bools(enc, held[2].data_ptr(), None, 64, 100)
    assert e.value.name == "INVALID_ARG"
    for call in (lambda: adam_pages.encode_strings(enc, None, None, None, 64, PAGE_ROWS),  # a null source with rows
                 lambda: adam_pages.encode_bools(enc, None, None, 64, PAGE_ROWS)):
        with pytest.raises(_capi.BQSRError) as e:
            call()
        assert e.value.name == "INVALID_ARG"
    check_bools(enc, np.ones(64, bool))  # (a size call and its emit)
    with pytest.raises(_capi.BQSRError) as e:
        _capi.check(PP._lib().bqsr_parquet_pages_emit(enc.h, None, None, None))  # no size call before it
    assert e.value.name == "INVALID_ARG"


# ---- end to end ----

HEADER = (b"@HD\tVN:1.4\tSO:unsorted\n@SQ\tSN:chr20\tLN:100000000\tUR:file:/ref.fa\n@SQ\tSN:chrM\tLN:16571\n"
          b"@RG\tID:rg0\tLB:lib0\tSM:s\tPI:250\tPL:ILLUMINA\tDT:2013-06-01T12:30:00Z\n@RG\tID:rg1\tSM:t\n")
# unmapped reads, `*` SEQ / QUAL, reads with and without tags and MD, mates on either reference
EXTRA = (b"u%d\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n",
         b"u%d\t77\t*\t0\t0\t*\t*\t0\t0\tACGTN\tIIII#\tRG:Z:rg1\n",
         b"m%d\t99\tchr20\t100\t60\t5M\t=\t300\t205\tACGTA\tIIIII\tMD:Z:5\tRG:Z:rg0\tNM:i:0\tXA:A:c\tXS:f:1.5\n",
         b"m%d\t147\tchr20\t300\t255\t2S3M\tchrM\t7\t0\tACGGT\t#IIII\tRG:Z:rg1\tMD:Z:3\n",
         b"n%d\t272\tchr20\t500\t30\t4M\t*\t0\t0\tGGGG\t????\n",  # (secondary: BQSR passes it through)
         b"s%d\t0\tchrM\t5\t3\t*\t*\t0\t0\t*\t*\tRG:Z:nope\n")


@functools.lru_cache(maxsize=None)
def e2e_text():
    """about 400 reads: generated mapped pairs in two read groups (rg1 without LB and PI), the EXTRA forms at part
    edges (part_reads 64) and in between"""
    b = synth.generate(384, (60,), 2, 11, contig_len=3000, p_duplicate=0.0)
    body = [l for l in sam_text(b, n_rg=2, qname="p").split(b"\n") if l and not l.startswith(b"@")]
    for k in range(1, len(body), 2):  # mates share a QNAME (MarkDuplicates has pairs to work on)
        f = body[k].split(b"\t")
        f[0] = body[k - 1].split(b"\t")[0]
        body[k] = b"\t".join(f)
    lines = [l + b"\n" for l in body]
    for j, at in enumerate((0, 63, 64, 65, 127, 128, 200, 201, 202, 255, 256, 300, 390)):
        lines.insert(at, EXTRA[j % len(EXTRA)] % j)
    return HEADER + b"".join(lines)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bytes_e2e")
    text = e2e_text()
    paths = {"sam": str(d / "in.sam"), "bam": str(d / "in.bam")}
    open(paths["sam"], "wb").write(text)
    open(paths["bam"], "wb").write(sam_to_bam(text))
    return paths


def both(tmp_path, inp, **kw):
    """the same transform call with the host and with the device encoder: (device table, parts, stats, path),
    after the comparisons every case shares"""
    host, out = str(tmp_path / "host.adam"), str(tmp_path / "dev.adam")
    transform(inp, host, **kw)
    st = transform(inp, out, parquet_encoder="device", **kw)
    got, parts = read_output(out)
    want, want_parts = read_output(host)
    assert parts == want_parts == st["parts"]
    assert got.schema.equals(want.schema) and got.schema.equals(adam_save.schema())
    assert got.equals(want)  # values and nulls
    return got, parts, st, out


@pytest.mark.parametrize("codec", ["gzip", "snappy", "none"])
@pytest.mark.parametrize("kind", ["sam", "bam"])
def test_transform_device_pages_equal_the_host_path(inputs, tmp_path, kind, codec):
    import pyarrow.parquet as pq
    got, parts, st, out = both(tmp_path, inputs[kind], part_reads=64, page_rows=PAGE_ROWS, compression=codec)
    assert got.num_rows == 397 and parts == 7
    # the input has what it is meant to have: nulls in a header column, unmapped reads, `*`, reads without tags
    assert 0 < got.column("recordGroupLibrary").null_count < got.num_rows
    assert 0 < got.column("recordGroupPredictedMedianInsertSize").null_count < got.num_rows
    assert got.column("referenceId").null_count and got.column("mismatchingPositions").null_count
    assert "*" in got.column("sequence").to_pylist() and "" in got.column("attributes").to_pylist()
    assert got.column("mateReference").null_count < got.num_rows
    assert st["pages"]["bytes_downloaded"] > 0 and st["pages"]["kernel_ms"]["emit"] > 0.0
    assert st["pages"]["file_bytes"] == sum(os.path.getsize(p) for p in glob.glob(os.path.join(out, "*")))
    first = os.path.join(out, "part-r-00000.parquet")
    host_first = os.path.join(str(tmp_path / "host.adam"), "part-r-00000.parquet")
    md, t = pq.ParquetFile(first).metadata.row_group(0), pq.read_table(first)
    hmd = pq.ParquetFile(host_first).metadata.row_group(0)
    for i in range(t.num_columns):
        assert md.column(i).compression == {"gzip": "GZIP", "snappy": "SNAPPY", "none": "UNCOMPRESSED"}[codec]
        assert md.column(i).statistics.null_count == t.column(i).null_count, t.column_names[i]
        assert md.column(i).physical_type == hmd.column(i).physical_type, t.column_names[i]
    kinds = dict(adam_save.ADAM_FIELDS)
    assert [md.column(i).physical_type for i in range(t.num_columns) if kinds[t.column_names[i]] == "bool"] == \
        ["BOOLEAN"] * 11
    for name in adam_save.STR_COLS:  # PLAIN BYTE_ARRAY, no dictionary page
        c = md.column(t.column_names.index(name))
        assert c.physical_type == "BYTE_ARRAY" and not c.has_dictionary_page


@pytest.mark.parametrize("case", ["markdup_recalibrate", "sort_reads", "partitions_recalibrate",
                                  "partitions_markdup"])
def test_transform_device_pages_other_paths(inputs, tmp_path, case):
    n_text = len(e2e_text())
    kw = {"markdup_recalibrate": dict(mark_duplicates=True, recalibrate=True),  # (the set_quals path)
          "sort_reads": dict(sort_reads=True),
          "partitions_recalibrate": dict(recalibrate=True, partition_bytes=n_text // 4),  # (the _partitions path)
          "partitions_markdup": dict(mark_duplicates=True, partition_bytes=n_text // 4)}[case]
    got, parts, st, _ = both(tmp_path, inputs["sam"], part_reads=64, page_rows=PAGE_ROWS, **kw)
    assert got.num_rows == 397
    if case.startswith("partitions"):
        assert st["partitions"] > 2 and parts >= 7
    if "markdup" in case:
        assert st["duplicates"] == sum(got.column("duplicateRead").to_pylist())


@pytest.mark.parametrize("name", FIXTURES)
def test_golden_fixtures_through_the_command_line(tmp_path, name):
    host, out = str(tmp_path / "host.adam"), str(tmp_path / "dev.adam")
    src = os.path.join(GOLD, name)
    assert transform_main([src, host, "-part_reads", "3"]) == 0
    assert transform_main([src, out, "-part_reads", "3", "-parquet_encoder", "device"]) == 0  # default page sizes
    got, want = read_output(out), read_output(host)
    assert got[1] == want[1] and want[0].num_rows > 0
    assert got[0].schema.equals(want[0].schema) and got[0].equals(want[0])


def test_no_reads_and_overwrite(tmp_path):
    import pyarrow.parquet as pq
    inp, host, out = str(tmp_path / "in.sam"), str(tmp_path / "host.adam"), str(tmp_path / "dev.adam")
    open(inp, "wb").write(HEADER)
    transform(inp, host)
    st = transform(inp, out, parquet_encoder="device")
    assert st["parts"] == 1
    got, want = read_output(out), read_output(host)
    assert got[1] == want[1] == 1 and got[0].num_rows == 0 and got[0].equals(want[0])
    assert got[0].schema.equals(adam_save.schema())
    a = pq.ParquetFile(os.path.join(out, "part-r-00000.parquet"))
    b = pq.ParquetFile(os.path.join(host, "part-r-00000.parquet"))
    assert a.schema.equals(b.schema)
    with pytest.raises(FileExistsError):
        transform(inp, out, parquet_encoder="device")
    transform(inp, out, parquet_encoder="device", overwrite=True)
    assert read_output(out)[0].num_rows == 0


def test_a_refused_tag_in_a_later_part_leaves_no_output(tmp_path):
    text = e2e_text()
    lines = text[len(HEADER):].splitlines(True)
    lines[333] = lines[333].rstrip(b"\n") + b"\tXB:B:c,1,2\n"  # the reference's attribute conversion throws
    bad, gone = str(tmp_path / "bad.sam"), str(tmp_path / "gone.adam")
    open(bad, "wb").write(HEADER + b"".join(lines))
    with pytest.raises(_capi.BQSRError) as e:
        transform(bad, gone, part_reads=64, page_rows=PAGE_ROWS, parquet_encoder="device")
    assert (e.value.name, e.value.read) == ("UNSUPPORTED", 333)
    assert not os.path.lexists(gone) and not os.path.lexists(gone + ".partial")
