"""adam_amd/parquet_pages.py's file assembly without a device: pages made by
the numpy restatement (tests/_parquet_pages_ref.py), put into a file by the
product's assembler, read back through pyarrow equal to the input arrays --
every index width, the three codecs, an empty table -- and the footer's schema
equal to the host path's."""
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import _parquet_pages_ref as R
from adam_amd import adam_save
from adam_amd import parquet_pages as PP

WIDTHS = (1, 5, 8, 9, 17, 32)
PAGE_ROWS = 128


def index_column(name, w, n, seed):
    """a dictionary column of int64 entries: (Column, expected pyarrow array)"""
    rng = np.random.default_rng(seed)
    entries = min(1 << w, 3000) if w < 32 else 3000
    dic = rng.integers(-1 << 40, 1 << 40, entries)
    valid = rng.random(n) > 0.25
    idx = rng.integers(0, entries, n)
    idx[64:64 + 200] = idx[64]  # runs of equal indices: RLE blocks between bit-packed ones
    if w > 1:
        idx[-1] = entries - 1
    bodies, pages = R.column_pages(R.DICT_INDEX, idx, valid, PAGE_ROWS, w)
    col = PP.Column(name, "int64", PP.Stream(np.frombuffer(bodies, np.uint8), pages), PP.plain_ints(dic, "int64"))
    return col, pa.array(dic[idx], pa.int64(), mask=~valid)


@pytest.mark.parametrize("codec", ["none", "snappy", "gzip"])
def test_every_width_reads_back(tmp_path, codec):
    n = 777
    fields, cols, want = [], [], []
    for w in WIDTHS:
        c, a = index_column("w%d" % w, w, n, w)
        fields.append((c.name, "int64"))
        cols.append(c)
        want.append(a)
    # (width 32 here with small indices -- indices that use its top bits would need a 2^31-entry dictionary; those
    # bytes are the device test's); a PLAIN int32, a PLAIN int64 and a string dictionary complete the forms
    rng = np.random.default_rng(99)
    for name, kind, typ in (("p32", R.PLAIN_INT32, "int32"), ("p64", R.PLAIN_INT64, "int64")):
        v = rng.integers(-1 << 30, 1 << 30, n) if typ == "int32" else rng.integers(-1 << 62, 1 << 62, n)
        ok = rng.random(n) > 0.5
        bodies, pages = R.column_pages(kind, v, ok, PAGE_ROWS)
        fields.append((name, typ))
        cols.append(PP.Column(name, typ, PP.Stream(np.frombuffer(bodies, np.uint8), pages)))
        want.append(pa.array(v, pa.int32() if typ == "int32" else pa.int64(), mask=~ok))
    words = ["", "A", "chr20", "é-ü", "x" * 300]
    idx, ok = rng.integers(0, len(words), n), rng.random(n) > 0.1
    bodies, pages = R.column_pages(R.DICT_INDEX, idx, ok, PAGE_ROWS, PP.bit_width(len(words)))
    fields.append(("s", "string"))
    cols.append(PP.Column("s", "string", PP.Stream(np.frombuffer(bodies, np.uint8), pages), PP.plain_strings(words)))
    want.append(pa.array([words[i] if o else None for i, o in zip(idx, ok)], pa.string()))
    path = str(tmp_path / "t.parquet")
    size = PP.assemble(path, fields, cols, n, None if codec == "none" else codec)
    assert size == os.path.getsize(path)
    got = pq.read_table(path)
    assert got.equals(pa.table(want, names=[f for f, _ in fields]))
    md = pq.ParquetFile(path).metadata
    assert md.num_rows == n and md.num_row_groups == 1
    for i, c in enumerate(cols):
        cm = md.row_group(0).column(i)
        assert cm.compression == {"none": "UNCOMPRESSED", "snappy": "SNAPPY", "gzip": "GZIP"}[codec]
        assert cm.statistics.null_count == want[i].null_count and not cm.statistics.has_min_max
        # format-1.0 names only, as Arrow's version="1.0" writer declares them
        assert set(cm.encodings) == ({"PLAIN_DICTIONARY", "RLE"} if c.dictionary else {"RLE", "PLAIN"})


def test_shared_stream_and_string_array_dictionary(tmp_path):
    n = 300
    idx = np.arange(n) % 7
    ok = np.arange(n) % 5 != 0
    bodies, pages = R.column_pages(R.DICT_INDEX, idx, ok, PAGE_ROWS, 3)
    st = PP.Stream(np.frombuffer(bodies, np.uint8), pages)
    names = pa.array(["r%d" % (i * i) for i in range(7)] + [""], pa.string())
    body, count = PP.plain_string_array(names.slice(0, 7))
    assert (bytes(body), count) == PP.plain_strings(names.to_pylist()[:7])
    cols = [PP.Column("a", "string", st, (body, count)),
            PP.Column("b", "int32", st, PP.plain_ints(range(10, 17), "int32"))]
    path = str(tmp_path / "t.parquet")
    PP.assemble(path, [("a", "string"), ("b", "int32")], cols, n, "snappy")
    got = pq.read_table(path)
    assert got.column("a").to_pylist() == ["r%d" % (i * i) if o else None for i, o in zip(idx, ok)]
    assert got.column("b").to_pylist() == [10 + int(i) if o else None for i, o in zip(idx, ok)]


def host_file(tmp_path, table):
    path = str(tmp_path / "host.parquet")
    pq.write_table(table, path, compression="snappy", use_dictionary=adam_save.PILEUP_DICT_COLS,
                   write_statistics=adam_save.PILEUP_STATS_COLS, store_schema=False)
    return path


def test_empty_table_and_schema_equal_the_host_path(tmp_path):
    host = host_file(tmp_path, adam_save.pileup_schema().empty_table())
    path = str(tmp_path / "t.parquet")
    PP.assemble(path, adam_save.PILEUP_FIELDS, [], 0, "gzip")
    got, want = pq.ParquetFile(path), pq.ParquetFile(host)
    assert got.schema.equals(want.schema)
    assert got.schema_arrow.equals(want.schema_arrow) and got.schema_arrow.equals(adam_save.pileup_schema())
    assert got.metadata.metadata is None or b"ARROW:schema" not in got.metadata.metadata
    for i in range(len(adam_save.PILEUP_FIELDS)):
        a, b = got.schema.column(i), want.schema.column(i)
        assert (a.name, a.physical_type, a.converted_type, a.max_definition_level, a.max_repetition_level) == \
            (b.name, b.physical_type, b.converted_type, b.max_definition_level, b.max_repetition_level)
    t = pq.read_table(path)
    assert t.num_rows == 0 and t.equals(pq.read_table(host))


def test_writer_follows_adam_writer_rules(tmp_path):
    out = str(tmp_path / "o.adam")
    bodies, pages = R.column_pages(R.PLAIN_INT32, np.arange(5), np.ones(5, bool), PAGE_ROWS)
    col = PP.Column("x", "int32", PP.Stream(np.frombuffer(bodies, np.uint8), pages))
    W = PP.PagesWriter(out, [("x", "int32")], "gzip")
    W.add([col], 5)
    W.add([col], 5)
    assert os.path.isdir(out + ".partial") and not os.path.exists(out)
    W.close(True)
    assert sorted(os.listdir(out)) == ["_SUCCESS", "part-r-00000.parquet", "part-r-00001.parquet"]
    assert adam_save.is_adam_output(out) and W.parts == 2 and W.rows == 10
    assert W.file_bytes == sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out))
    assert pq.read_table(os.path.join(out, "part-r-00001.parquet")).column("x").to_pylist() == list(range(5))
    with pytest.raises(FileExistsError):
        PP.PagesWriter(out, [("x", "int32")])
    W = PP.PagesWriter(out, [("x", "int32")], overwrite=True)
    W.add([col], 5)
    W.close(False)  # a failed job: nothing of it stays, the earlier output does
    assert not os.path.exists(out + ".partial") and len(os.listdir(out)) == 3


def test_restatement_bytes():
    """the forms, spelled out by hand once"""
    assert R.levels([1, 0, 1, 1, 0, 0, 0, 0, 1]) == bytes([3, 0, 0, 0, 0x05, 0b00001101, 0b00000001])
    assert R.indices([5] * 64, 3) == bytes([3, 0x80, 0x01, 5])
    assert R.indices([5] * 63 + [4], 3)[:2] == bytes([3, 0x11]) and len(R.indices([5] * 63 + [4], 3)) == 2 + 24
    assert R.indices([1, 2, 3], 2) == bytes([2, 0x03, 0b00111001, 0])
    assert R.indices([0x1FF] * 64 + [1], 9) == bytes([9, 0x80, 0x01, 0xFF, 0x01, 0x03, 1] + [0] * 8)
    assert PP.bit_width(1) == 1 and PP.bit_width(2) == 1 and PP.bit_width(17) == 5 and PP.bit_width(257) == 9
