"""Page bodies compressed with snappy on the device (adam_amd/csrc/
snappy_pages.hip through bqsr_snappy_pages and the encoder's compress / fetch)
against an independent decoder and the declared format (_snappy_cases.py): the
same bytes from two runs and from the block routine compiled for the host; the
encoder path for one column of each kind; `reads2ref` and `transform` with
-parquet_compressor device end to end."""
import functools
import glob
import os

import numpy as np
import pyarrow as pa
import pytest

import _parquet_bytes_ref as B
import _parquet_pages_ref as R
import _snappy_cases as C
from adam_amd import adam_pages, bqsr, reads2ref, synth
from adam_amd import parquet_pages as PP
from adam_amd.samgen import sam_text
from adam_amd.transform import transform

pytestmark = pytest.mark.gpu


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def run(data, off):
    """pages through the device, every check, the host routine's bytes, a second run's; returns the pages"""
    out, out_off = PP.snappy_pages(data, off)
    pages = C.check(out, out_off, data, off)
    host, host_off = PP.snappy_pages_host(data, off)
    assert out.tobytes() == host.tobytes() and np.array_equal(out_off, host_off), "the host-compiled routine differs"
    again, again_off = PP.snappy_pages(data, off)
    assert again.tobytes() == out.tobytes() and np.array_equal(again_off, out_off), "two runs differ"
    return pages


@pytest.mark.parametrize("kind", ["random", "zeros"])
@pytest.mark.parametrize("n", C.SIZES)
def test_sizes(n, kind):
    page, = run(C.random_bytes(n, 100 + n) if kind == "random" else bytes(n), [0, n])
    C.check_sizes(kind, len(page), n)


@pytest.mark.parametrize("name", C.CONTENTS)
def test_contents(name):
    data = C.content(name)
    page, = run(data, [0, len(data)])
    C.check_sizes(name, len(page), len(data))
    assert len(page) / C.pa_size(data) <= C.PINS[name]


def test_several_pages_at_odd_offsets():
    data, off = C.multi_pages()
    pages = run(data, off)
    assert [len(p) > 0 for p in pages] == [True] * 5 and pages[2] == b"\x00"
    # a window of a larger buffer: the first page starts at an odd offset of the input
    out, out_off = PP.snappy_pages(data, off[1:3])
    assert out.tobytes() == pages[1] and out_off.tolist() == [0, len(pages[1])]


def test_more_jobs_than_workgroups():
    """600 blocks of differing compressible content in pages of 1 to 5 blocks (the last block of a page short):
    above two jobs per CU of a 256-CU part, so the persistent loop runs"""
    rng = np.random.default_rng(11)
    sizes, blocks = [], 0
    while blocks < 600:
        k = min(1 + len(sizes) % 5, 600 - blocks)
        sizes.append(k * C.BLOCK - int(rng.integers(0, 3000)))
        blocks += k
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(off[-1])
    data = (rng.integers(0, 4, n, dtype=np.uint8) * rng.integers(0, 2, n, dtype=np.uint8) + 65).astype(np.uint8)
    data[::97] = rng.integers(0, 256, len(data[::97]), dtype=np.uint8)
    out, out_off = PP.snappy_pages(data, off)
    assert out_off[0] == 0 and out_off[-1] == len(out) and len(out) < n // 2
    raw, buf = data.tobytes(), out.tobytes()
    for i in range(len(sizes)):
        page = buf[out_off[i]:out_off[i + 1]]
        assert pa.decompress(page, decompressed_size=sizes[i], codec="snappy", asbytes=True) == raw[off[i]:off[i + 1]]
    # the format and the host routine's bytes on a sample: the first pages of every size, and the last page
    for i in list(range(5)) + [len(sizes) - 1]:
        page = buf[out_off[i]:out_off[i + 1]]
        assert C.walk(page, sizes[i]) == raw[off[i]:off[i + 1]]
        assert PP.snappy_pages_host(data, off[i:i + 2])[0].tobytes() == page
    snappy_ms, pack_ms = PP.compress_times()
    assert snappy_ms > 0.0 and pack_ms > 0.0


def test_output_that_does_not_fit():
    import ctypes
    from adam_amd import _capi
    L, ctx = PP._lib(), bqsr.Context.get(0)
    data = np.frombuffer(C.content("x16") + C.content("skewed"), np.uint8)
    off = np.array([0, 65280, 70001, len(data)], np.int64)
    want, want_off = PP.snappy_pages_host(data, off)
    out, got = np.zeros(len(want), np.uint8), np.zeros(4, np.int64)
    args = (ctx.handle, data.ctypes.data, off.ctypes.data_as(_capi.i64p), 3, None, out.ctypes.data)
    rc = L.bqsr_snappy_pages(*args, len(want) - 1, got.ctypes.data_as(_capi.i64p))
    assert rc == _capi.INVALID_ARG and got[3] == len(want) and not out.any()
    assert L.bqsr_snappy_pages(*args, len(want), got.ctypes.data_as(_capi.i64p)) == 0
    assert out.tobytes() == want.tobytes() and np.array_equal(got, want_off)
    assert ctypes.c_int64(got[3]).value <= sum(32 + n + n // 6 for n in np.diff(off))


# ---- the encoder path ----

@pytest.fixture(scope="module")
def encoders():
    ctx = bqsr.Context.get(0)
    host, device = PP.Encoder(ctx), PP.Encoder(ctx, compressor="device")
    yield host, device
    host.close()
    device.close()


def both(encoders, encode):
    """the same column through emit and through compress + fetch: the compressed pages are the host routine's of
    emit's bodies, the page table is emit's"""
    host, device = encoders
    down = device.bytes_down
    want, got = encode(host), encode(device)
    assert got.bodies is None and got.codec == "snappy"
    assert np.array_equal(got.pages, want.pages) and len(want.pages) > 1
    off = np.r_[want.pages[:, 0], want.pages[-1, 0] + want.pages[-1, 1]]
    comp, comp_off = PP.snappy_pages_host(np.asarray(want.bodies), off)
    assert np.array_equal(got.comp_off, comp_off) and got.comp.tobytes() == comp.tobytes()
    C.check(got.comp, got.comp_off, np.asarray(want.bodies), off)
    items = len(want.pages) + int(((want.pages[:, 1] + C.BLOCK - 1) // C.BLOCK).sum())  # varints and blocks
    assert device.bytes_down - down == len(comp) + got.pages.nbytes + 8 * (items + 1)
    assert all(device.ms[k] > 0.0 for k in PP.KERNELS + PP.CODEC_KERNELS)
    return want, got


def test_encoder_plain_int64(encoders):
    n = 20000
    v = np.arange(n, dtype=np.int64) * 3 + 1000000
    valid = np.arange(n) % 11 != 0
    held = [dev(v), dev(R.bitmap_words(valid).view(np.int64))]
    col = PP.ParquetColumn(kind=PP.PLAIN_INT64, src_width=8, src=held[0].data_ptr(), src_n=n,
                           validity=held[1].data_ptr())
    want, got = both(encoders, lambda e: e.encode(col, n, 16384))  # a full page holds 119 KB of values: 2 blocks
    assert want.pages[0, 1] > C.BLOCK and got.comp_off[-1] < want.pages[:, 1].sum()


def test_encoder_dict_index_with_nulls(encoders):
    rng = np.random.default_rng(4)
    n = 5000
    v = (rng.integers(0, 300, n) * (rng.random(n) > 0.5)).astype(np.int32)
    valid = rng.random(n) > 0.3
    held = [dev(v), dev(R.bitmap_words(valid).view(np.int64))]
    col = PP.ParquetColumn(kind=PP.DICT_INDEX, src_width=4, src=held[0].data_ptr(), src_n=n, bit_width=9,
                           validity=held[1].data_ptr())
    both(encoders, lambda e: e.encode(col, n, 1024))


def test_encoder_strings_with_a_page_above_one_block(encoders):
    rng = np.random.default_rng(6)
    n = 2500
    strings = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 100)) for _ in range(n)]
    valid = np.arange(n) % 17 != 3
    off, data, _ = B.arrow_strings(strings)
    held = [dev(off), dev(data), dev(R.bitmap_words(valid).view(np.int64))]
    want, got = both(encoders, lambda e: adam_pages.encode_strings(e, held[0].data_ptr(), held[1].data_ptr(),
                                                                   held[2].data_ptr(), n, 1024))
    assert want.pages[0, 1] > C.BLOCK  # 1024 rows of 104 bytes


def test_encoder_booleans(encoders):
    rng = np.random.default_rng(8)
    n = 70000
    bits = rng.random(n) > 0.9
    held = [dev(R.bitmap_words(bits).view(np.int64))]
    both(encoders, lambda e: adam_pages.encode_bools(e, held[0].data_ptr(), None, n, 65536))


def test_encoder_call_order(encoders):
    """one compress + fetch per size call; no emit after a compress, no fetch without one; only snappy"""
    import ctypes
    from adam_amd import _capi
    L = PP._lib()
    _, device = encoders
    held = [dev(np.arange(256, dtype=np.int32))]
    col = PP.ParquetColumn(kind=PP.PLAIN_INT32, src_width=4, src=held[0].data_ptr(), src_n=256)
    sz, n = PP.PagesSizes(), ctypes.c_int64()
    out, pages, off = np.zeros(4096, np.uint8), np.zeros((2, 4), np.int64), np.zeros(3, np.int64)
    offp = off.ctypes.data_as(_capi.i64p)

    def size():
        _capi.check(L.bqsr_parquet_pages_size(device.h, ctypes.byref(col), 256, 128, None, ctypes.byref(sz)))
    assert L.bqsr_parquet_pages_compress(device.h, PP.CODEC_SNAPPY, None, ctypes.byref(n)) == _capi.INVALID_ARG
    size()
    assert L.bqsr_parquet_pages_fetch(device.h, out.ctypes.data, pages.ctypes.data, offp, None) == _capi.INVALID_ARG
    assert L.bqsr_parquet_pages_compress(device.h, 2, None, ctypes.byref(n)) == _capi.INVALID_ARG
    assert L.bqsr_parquet_pages_compress(device.h, PP.CODEC_SNAPPY, None, ctypes.byref(n)) == 0 and n.value > 0
    assert L.bqsr_parquet_pages_emit(device.h, out.ctypes.data, pages.ctypes.data, None) == _capi.INVALID_ARG
    assert L.bqsr_parquet_pages_compress(device.h, PP.CODEC_SNAPPY, None, ctypes.byref(n)) == _capi.INVALID_ARG
    assert L.bqsr_parquet_pages_fetch(device.h, out.ctypes.data, pages.ctypes.data, offp, None) == 0
    assert off[2] == n.value and pages[:, 1].tolist() == [4 + 1 + 16 + 512] * 2
    assert L.bqsr_parquet_pages_fetch(device.h, out.ctypes.data, pages.ctypes.data, offp, None) == _capi.INVALID_ARG
    size()  # a size call after a compress drops what was not fetched
    _capi.check(L.bqsr_parquet_pages_compress(device.h, PP.CODEC_SNAPPY, None, ctypes.byref(n)))
    size()
    assert L.bqsr_parquet_pages_fetch(device.h, out.ctypes.data, pages.ctypes.data, offp, None) == _capi.INVALID_ARG
    _capi.check(L.bqsr_parquet_pages_emit(device.h, out.ctypes.data, pages.ctypes.data, None))


# ---- end to end ----

@functools.lru_cache(maxsize=None)
def e2e_text() -> bytes:
    """small_realignment_targets.sam plus 20 000 generated reads, under the two headers merged"""
    with open(os.path.join(C.GOLD, "small_realignment_targets.sam"), "rb") as fh:
        real = fh.read().splitlines(True)
    made = sam_text(synth.generate(20000, (100,), 2, 13), n_rg=2).splitlines(True)
    lines = real + made
    head = [l for l in lines if l.startswith(b"@") and not l.startswith(b"@HD")]
    order = {b"@SQ": 0, b"@RG": 1}
    head.sort(key=lambda l: order[l[:3]])
    return b"@HD\tVN:1.4\tSO:unsorted\n" + b"".join(head) + b"".join(l for l in lines if not l.startswith(b"@"))


def read_output(path):
    import pyarrow.parquet as pq
    parts = sorted(glob.glob(os.path.join(path, "part-r-*.parquet")))
    assert parts and os.path.exists(os.path.join(path, "_SUCCESS")) and not os.path.lexists(path + ".partial")
    for p in parts:  # every column chunk, so every data page, is SNAPPY
        md = pq.ParquetFile(p).metadata
        for g in range(md.num_row_groups):
            assert {md.row_group(g).column(i).compression for i in range(md.num_columns)} == {"SNAPPY"}
    return pa.concat_tables([pq.read_table(p) for p in parts]), len(parts)


@pytest.mark.parametrize("command", ["reads2ref", "transform"])
def test_end_to_end(tmp_path, command):
    inp = str(tmp_path / "in.sam")
    with open(inp, "wb") as fh:
        fh.write(e2e_text())
    stats = {}
    for compressor in ("host", "device"):
        out = str(tmp_path / (compressor + ".adam"))
        if command == "reads2ref":
            st = reads2ref.reads2ref(inp, out, compression="snappy", part_reads=8192, parquet_encoder="device",
                                     parquet_compressor=compressor)
            stats[compressor] = st["page_bytes_downloaded"], st["page_kernels_ms"]
        else:
            st = transform(inp, out, compression="snappy", part_reads=8192, parquet_encoder="device",
                           parquet_compressor=compressor)
            stats[compressor] = st["pages"]["bytes_downloaded"], st["pages"]["kernel_ms"]
    got, want = read_output(str(tmp_path / "device.adam")), read_output(str(tmp_path / "host.adam"))
    assert got[1] == want[1] > 1 and want[0].num_rows >= 20000
    assert got[0].schema.equals(want[0].schema) and got[0].equals(want[0])
    print("bytes downloaded: host compressor %d, device compressor %d" % (stats["host"][0], stats["device"][0]))
    assert 0 < stats["device"][0] < stats["host"][0]
    assert set(stats["host"][1]) == set(PP.KERNELS) and set(stats["device"][1]) == set(PP.KERNELS + PP.CODEC_KERNELS)
    assert stats["device"][1]["snappy"] > 0.0 and stats["device"][1]["pack"] > 0.0


def test_the_command_line_flag(tmp_path):
    src = os.path.join(C.GOLD, "small_realignment_targets.sam")
    host, out = str(tmp_path / "host.adam"), str(tmp_path / "dev.adam")
    flags = ["-parquet_encoder", "device", "-parquet_compression", "snappy"]
    assert reads2ref.main([src, host] + flags) == 0
    assert reads2ref.main([src, out] + flags + ["-parquet_compressor", "device"]) == 0
    assert read_output(out)[0].equals(read_output(host)[0])
