"""The snappy page codec without a GPU: the block routine of
adam_amd/csrc/snappy_pages.hip compiled for the host (bqsr_snappy_pages_host)
against an independent decoder and the declared format (_snappy_cases.py), the
new entry points' argument checks, parquet_pages.assemble over streams that
arrive compressed, and the refusals of -parquet_compressor device."""
import ctypes
import os
import threading

import numpy as np
import pytest

import _parquet_pages_ref as R
import _snappy_cases as C
from adam_amd import _capi, reads2ref, transform
from adam_amd import parquet_pages as PP

SAM = os.path.join(C.GOLD, "small_realignment_targets.sam")


def run(data: bytes):
    """one page through the host routine and every check; returns the compressed page"""
    out, off = PP.snappy_pages_host(data, [0, len(data)])
    page, = C.check(out, off, data, [0, len(data)])
    return page


@pytest.mark.parametrize("kind", ["random", "zeros"])
@pytest.mark.parametrize("n", C.SIZES)
def test_sizes(n, kind):
    page = run(C.random_bytes(n, 100 + n) if kind == "random" else bytes(n))
    C.check_sizes(kind, len(page), n)


@pytest.mark.parametrize("name", C.CONTENTS)
def test_contents(name):
    data = C.content(name)
    assert len(data) == (2 * C.BLOCK if name == "random_x2" else len(data)) and len(data) <= 2 * C.BLOCK
    page = run(data)
    C.check_sizes(name, len(page), len(data))
    ratio = len(page) / C.pa_size(data)
    print("size pin %s: %d bytes, pyarrow snappy %d, ratio %.4f" % (name, len(page), C.pa_size(data), ratio))
    assert ratio <= C.PINS[name]


def test_copy_forms_at_the_offset_boundary():
    """8 bytes, zeros, the 8 bytes again: the repeat is one copy at its distance, in the 1-byte-offset form
    below 2048 and in the 2-byte-offset form from there"""
    x = C.random_bytes(8, 41)
    for dist, form in ((2047, 1), (2048, 2), (65528, 2)):
        data = x + bytes(dist - 8) + x + bytes([x[0] ^ 255])
        got = [c for c in copies_of(data) if c[1] == dist]
        assert got == [(8, dist, form)], (dist, got)
    # and a long match below 2048 takes the 2-byte form
    x = C.random_bytes(12, 43)
    assert [c for c in copies_of(x + bytes(100) + x + bytes([x[0] ^ 255])) if c[1] == 112] == [(12, 112, 2)]


def copies_of(data: bytes):
    """(length, offset, offset bytes) of the copy elements of one small page"""
    page = run(data)
    at, res = len(R.varint(len(data))), []
    while at < len(page):
        tag = page[at]
        if tag & 3 == 0:
            ln = tag >> 2
            extra = max(0, ln - 59)
            ln = int.from_bytes(page[at + 1:at + 1 + extra], "little") if extra else ln
            at += 1 + extra + ln + 1
        elif tag & 3 == 1:
            res.append((4 + ((tag >> 2) & 7), ((tag >> 5) << 8) | page[at + 1], 1))
            at += 2
        else:
            res.append(((tag >> 2) + 1, page[at + 1] | (page[at + 2] << 8), 2))
            at += 3
    return res


def test_several_pages_at_odd_offsets():
    data, off = C.multi_pages()
    out, out_off = PP.snappy_pages_host(data, off)
    pages = C.check(out, out_off, data, off)
    assert pages[2] == b"\x00"
    # a page's bytes do not depend on its neighbours or its offset
    for i in range(len(C.MULTI)):
        one = data[off[i]:off[i + 1]].copy()
        assert PP.snappy_pages_host(one, [0, len(one)])[0].tobytes() == pages[i]
    # a window of a larger buffer: offsets that do not start at 0
    out2, off2 = PP.snappy_pages_host(data, off[1:3])
    assert out2.tobytes() == pages[1] and off2.tolist() == [0, len(pages[1])]
    again, again_off = PP.snappy_pages_host(data, off)
    assert again.tobytes() == out.tobytes() and np.array_equal(again_off, out_off)


def test_output_that_does_not_fit():
    L = PP._lib()
    data = np.frombuffer(C.content("x16") + C.content("skewed"), np.uint8)
    off = np.array([0, 65280, 70000, len(data)], np.int64)
    want, want_off = PP.snappy_pages_host(data, off)
    out = np.zeros(len(want), np.uint8)
    got = np.zeros(4, np.int64)
    args = (data.ctypes.data, off.ctypes.data_as(_capi.i64p), 3, out.ctypes.data)
    rc = L.bqsr_snappy_pages_host(*args, len(want) - 1, got.ctypes.data_as(_capi.i64p))
    assert rc == _capi.INVALID_ARG and got[3] == len(want)
    assert L.bqsr_snappy_pages_host(*args, len(want), got.ctypes.data_as(_capi.i64p)) == 0
    assert out.tobytes() == want.tobytes() and np.array_equal(got, want_off)


def test_exports_and_argument_checks():
    L = PP._lib()
    for name in ("bqsr_snappy_pages", "bqsr_snappy_pages_host", "bqsr_parquet_pages_compress",
                 "bqsr_parquet_pages_fetch", "bqsr_parquet_pages_compress_times"):
        assert hasattr(L, name), name
    data = np.arange(100, dtype=np.uint8)
    out, oo = np.zeros(200, np.uint8), np.zeros(3, np.int64)
    oop = oo.ctypes.data_as(_capi.i64p)

    def host(in_, off, n_pages, out_, cap, oo_):
        offp = None if off is None else np.asarray(off, np.int64).ctypes.data_as(_capi.i64p)
        return L.bqsr_snappy_pages_host(in_, offp, n_pages, out_, cap, oo_)
    d, o = data.ctypes.data, out.ctypes.data
    assert host(d, [0, 50, 100], 2, o, 200, oop) == 0 and oo[2] > 0
    assert host(d, [0, 50, 100], -1, o, 200, oop) == _capi.INVALID_ARG
    assert host(d, None, 2, o, 200, oop) == _capi.INVALID_ARG
    assert host(d, [0, 50, 100], 2, o, 200, None) == _capi.INVALID_ARG
    assert host(d, [0, 50, 100], 2, None, 200, oop) == _capi.INVALID_ARG
    assert host(d, [0, 50, 100], 2, o, -1, oop) == _capi.INVALID_ARG
    assert host(d, [0, 60, 50], 2, o, 200, oop) == _capi.INVALID_ARG   # decreasing
    assert host(d, [-1, 50, 100], 2, o, 200, oop) == _capi.INVALID_ARG
    assert host(None, [0, 50, 100], 2, o, 200, oop) == _capi.INVALID_ARG
    assert host(None, [7, 7, 7], 2, o, 200, oop) == 0 and out[:2].tolist() == [0, 0] and oo.tolist() == [0, 1, 2]
    assert host(None, [0], 0, None, 0, oop) == 0 and oo[0] == 0
    # the device entry points refuse a null context / handle before they touch a device
    offp = np.array([0, 50, 100], np.int64).ctypes.data_as(_capi.i64p)
    assert L.bqsr_snappy_pages(None, d, offp, 2, None, o, 200, oop) == _capi.INVALID_ARG
    n = ctypes.c_int64()
    assert L.bqsr_parquet_pages_compress(None, PP.CODEC_SNAPPY, None, ctypes.byref(n)) == _capi.INVALID_ARG
    assert L.bqsr_parquet_pages_fetch(None, o, None, oop, None) == _capi.INVALID_ARG
    seen = []  # a thread that ran no compress reads zeros
    t = threading.Thread(target=lambda: seen.append(PP.compress_times()))
    t.start()
    t.join()
    assert seen == [(0.0, 0.0)]
    with pytest.raises(ValueError):
        PP.Encoder(None, compressor="elsewhere")


def _columns(compressed: bool):
    """three columns of 300 rows in 128-row pages, built by the numpy restatement: PLAIN int64 with nulls, a
    dictionary int32 column, and two string columns over one shared index stream"""
    rng = np.random.default_rng(5)
    n = 300
    valid = rng.random(n) > 0.2

    def stream(kind, values, ok, w=0):
        bodies, pages = R.column_pages(kind, values, ok, 128, w)
        bodies = np.frombuffer(bodies, np.uint8)
        if not compressed:
            return PP.Stream(bodies, pages)
        comp, comp_off = PP.snappy_pages_host(bodies, np.r_[pages[:, 0], pages[-1, 0] + pages[-1, 1]])
        return PP.Stream(None, pages, comp, comp_off, "snappy")
    idx = stream(R.DICT_INDEX, rng.integers(0, 5, n), np.ones(n, bool), 3)
    names = PP.plain_strings(["a", "bb", "ccc", "dddd", "eeeee"])
    return n, [("x", "int64"), ("k", "int32"), ("s", "string"), ("t", "string")], [
        PP.Column("x", "int64", stream(R.PLAIN_INT64, rng.integers(0, 1 << 40, n) // 7 * 7, valid)),
        PP.Column("k", "int32", stream(R.DICT_INDEX, rng.integers(0, 9, n), valid, 4),
                  PP.plain_ints(np.arange(100, 109), "int32")),
        PP.Column("s", "string", idx, names), PP.Column("t", "string", idx, names)]


def test_assemble_takes_compressed_streams(tmp_path):
    import pyarrow.parquet as pq
    tables = {}
    for compressed in (False, True):
        n, fields, cols = _columns(compressed)
        path = str(tmp_path / ("c%d.parquet" % compressed))
        size = PP.assemble(path, fields, cols, n, "snappy")
        assert size == os.path.getsize(path)
        tables[compressed] = pq.read_table(path)
        md = pq.ParquetFile(path).metadata.row_group(0)
        assert [md.column(i).compression for i in range(md.num_columns)] == ["SNAPPY"] * 4
    assert tables[True].num_rows == 300 and tables[True].column("x").null_count > 0
    assert tables[True].schema.equals(tables[False].schema) and tables[True].equals(tables[False])
    # a stream compressed for another codec than the file's is refused
    n, fields, cols = _columns(True)
    with pytest.raises(ValueError):
        PP.assemble(str(tmp_path / "bad.parquet"), fields, cols, n, "gzip")


@pytest.mark.parametrize("encoder,codec,why", [("host", "snappy", PP.COMPRESSOR_NEEDS_ENCODER),
                                               ("device", "gzip", PP.COMPRESSOR_NEEDS_SNAPPY),
                                               ("device", "none", PP.COMPRESSOR_NEEDS_SNAPPY)])
def test_refusals_of_the_device_compressor(tmp_path, capsys, encoder, codec, why):
    r2r, tr = str(tmp_path / "r2r.adam"), str(tmp_path / "tr.adam")
    with pytest.raises(ValueError) as e:
        reads2ref.reads2ref(SAM, r2r, compression=codec, parquet_encoder=encoder, parquet_compressor="device")
    assert str(e.value) == why
    with pytest.raises(ValueError) as e:
        transform.transform(SAM, tr, compression=codec, parquet_encoder=encoder, parquet_compressor="device")
    assert str(e.value) == why
    for main, out in ((reads2ref.main, r2r), (transform.main, tr)):
        with pytest.raises(SystemExit) as e:
            main([SAM, out, "-parquet_encoder", encoder, "-parquet_compression", codec, "-parquet_compressor",
                  "device"])
        assert e.value.code == 2 and why in capsys.readouterr().err.replace("\n", " ")
    with pytest.raises(ValueError) as e:
        reads2ref.reads2ref(SAM, r2r, compression="snappy", parquet_encoder="device", parquet_compressor="gpu")
    assert str(e.value) == PP.COMPRESSOR_CHOICE
    assert os.listdir(str(tmp_path)) == []  # nothing created, not even a .partial
