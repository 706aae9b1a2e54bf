"""Inputs and checks shared by the device snappy tests (snappy_pages.hip):
test_snappy_host.py runs them through the block routine compiled for the host
(parquet_pages.snappy_pages_host), test_gpu_snappy_pages.py through the device.

The oracle for a compressor is an independent decoder: every page is
decompressed by pyarrow's snappy, and walked element by element by the small
decoder below, which also asserts the format include/adam_sam.h declares.  The
size conditions compare with pyarrow's snappy on the same bytes."""
import functools
import os

import numpy as np
import pyarrow as pa

import _parquet_pages_ref as R

BLOCK = 65536
GOLD = os.path.join(os.path.dirname(__file__), "golden", "reference_resources")

SIZES = [0, 1, 3, 4, 5, 59, 60, 61, 64, 65, 68, 255, 256, 257, 2047, 2048, 2049, 65535, 65536, 65537, 131072, 131073]


def random_bytes(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _far(dist: int) -> bytes:
    """a 300-byte string, and again `dist` bytes later"""
    x = random_bytes(300, 21)
    return x + random_bytes(dist - 300, 22) + x


@functools.lru_cache(maxsize=None)
def real_page() -> bytes:
    """the PLAIN BYTE_ARRAY `sequence` page body of small_realignment_targets.sam: the levels as
    _parquet_pages_ref builds them, then a u32 length and the bytes of every present sequence"""
    seqs = []
    with open(os.path.join(GOLD, "small_realignment_targets.sam"), "rb") as fh:
        for line in fh:
            if not line.startswith(b"@"):
                seqs.append(line.rstrip(b"\n").split(b"\t")[9])
    ok = [s != b"*" for s in seqs]
    return R.levels(ok) + b"".join(len(s).to_bytes(4, "little") + s for s, k in zip(seqs, ok) if k)


def content(name: str) -> bytes:
    if name == "zeros":
        return bytes(BLOCK)
    if name == "random":
        return random_bytes(BLOCK, 5)
    if name == "one_byte":
        return b"\x41" * BLOCK
    if name == "period2":
        return b"\x41\x5a" * (BLOCK // 2)
    if name == "x16":
        return random_bytes(4080, 6) * 16
    if name == "skewed":
        p = 0.75 ** np.arange(64)
        return np.random.default_rng(7).choice(64, BLOCK, p=p / p.sum()).astype(np.uint8).tobytes()
    if name == "far2047":
        return _far(2047)
    if name == "far2048":
        return _far(2048)
    if name == "far65535":
        return _far(65535)
    if name == "random_x2":
        return random_bytes(BLOCK, 8) * 2
    if name == "real_page":
        return real_page()
    raise KeyError(name)


CONTENTS = ["zeros", "random", "one_byte", "period2", "x16", "skewed", "far2047", "far2048", "far65535", "random_x2",
            "real_page"]

# pages of 1, 65537, 0, 7 and 131073 bytes laid end to end: odd offsets, an empty page, pages of 1, 2 and 3 blocks
MULTI = [1, 65537, 0, 7, 131073]


def multi_pages():
    """(data, offsets) of the MULTI pages, compressible and not"""
    rng = np.random.default_rng(31)
    off = np.concatenate([[0], np.cumsum(MULTI)]).astype(np.int64)
    n = int(off[-1])
    data = (rng.integers(0, 4, n, dtype=np.uint8) * rng.integers(0, 2, n, dtype=np.uint8) + 65).astype(np.uint8)
    data[70000:90000] = rng.integers(0, 256, 20000, dtype=np.uint8)
    return data, off


def _varint(buf: bytes, at: int):
    v, shift = 0, 0
    while True:
        b = buf[at]
        at += 1
        v |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            return v, at
        assert shift < 35, "varint too long"


def walk(page: bytes, n: int) -> bytes:
    """Decode one compressed page element by element, asserting the declared
    format: varint(n); the blocks' elements end exactly at 65536-byte
    boundaries of the output; no 4-byte-offset copy; copy lengths 4..64; an
    offset at most the position within the block; the 1-byte-offset form
    exactly when length <= 11 and offset < 2048; no two adjacent literal
    elements inside a block; the shortest literal length form."""
    got, at = _varint(page, 0)
    assert got == n and page[:at] == R.varint(n), "the length varint"
    out = bytearray()
    prev_literal = False
    while at < len(page):
        in_block = len(out) % BLOCK
        if in_block == 0:
            prev_literal = False  # a new block: its first element may be a literal after a literal
        room = min(BLOCK, n - (len(out) - in_block)) - in_block  # bytes left in this block
        tag = page[at]
        kind = tag & 3
        if kind == 0:
            assert not prev_literal, "two adjacent literal elements in a block"
            ln = tag >> 2
            at += 1
            if ln >= 60:
                extra = ln - 59
                assert extra <= 2, "a literal longer than a block"
                ln = int.from_bytes(page[at:at + extra], "little")
                at += extra
                assert ln + 1 > (60 if extra == 1 else 256), "a literal length in a longer form than it needs"
            ln += 1
            assert ln <= room, "a literal crosses a block boundary"
            assert at + ln <= len(page)
            out += page[at:at + ln]
            at += ln
            prev_literal = True
            continue
        assert kind != 3, "a 4-byte-offset copy"
        if kind == 1:
            ln = 4 + ((tag >> 2) & 7)
            off = ((tag >> 5) << 8) | page[at + 1]
            at += 2
        else:
            ln = (tag >> 2) + 1
            off = page[at + 1] | (page[at + 2] << 8)
            at += 3
        assert 4 <= ln <= 64, "copy length %d" % ln
        assert 1 <= off <= in_block, "a copy reaches before its block (offset %d at %d)" % (off, in_block)
        assert ln <= room, "a copy crosses a block boundary"
        assert (kind == 1) == (ln <= 11 and off < 2048), "the copy form"
        for _ in range(ln):  # (byte by byte: copies overlap)
            out.append(out[-off])
        prev_literal = False
    assert at == len(page) and len(out) == n
    return bytes(out)


def check(out, out_off, data, page_off):
    """every page of the packed output `out` (offsets out_off) of the pages
    data[page_off[i]:page_off[i + 1]]: pyarrow's decoder, the walker, the size
    bound.  Returns the compressed pages."""
    out, data = bytes(out), bytes(data)
    assert len(out_off) == len(page_off) and out_off[0] == 0 and out_off[-1] == len(out)
    pages = []
    for i in range(len(page_off) - 1):
        raw = data[page_off[i]:page_off[i + 1]]
        page = out[out_off[i]:out_off[i + 1]]
        n = len(raw)
        if n:  # (pyarrow refuses a zero-size output buffer)
            assert pa.decompress(page, decompressed_size=n, codec="snappy", asbytes=True) == raw
        else:
            assert page == b"\x00"
        assert walk(page, n) == raw
        assert len(page) <= 32 + n + n // 6
        pages.append(page)
    return pages


def check_sizes(name: str, size: int, n: int):
    """the derived size conditions of the named contents"""
    if name in ("zeros", "one_byte"):
        assert size <= n // 16 + 16
    if name == "random":  # per block; the few accidental 4-byte matches of a random block cost 2 bytes each
        assert size <= sum(b + b // 1000 + 16 for b in [BLOCK] * (n // BLOCK) + [n % BLOCK])
    if name == "x16":
        assert size < n // 8
    if name == "random_x2":  # two blocks of the same 65536 bytes: the second cannot see the first
        assert n == 2 * BLOCK and size > 1.9 * BLOCK


def pa_size(data: bytes) -> int:
    return len(pa.compress(data, codec="snappy", asbytes=True))


# This codec's size / pyarrow's snappy size, measured on the first run of the
# host-compiled routine and rounded up to one decimal (the output is a function
# of the input alone, so a figure moves only when the kernel or pyarrow's snappy
# does): zeros 1.000 (3077 / 3077 bytes), random 1.000 (65542 / 65542), one_byte
# 1.000 (3077 / 3077), period2 1.000 (3078 / 3078), x16 1.088 (7654 / 7037),
# skewed 0.977 (48677 / 49844), far2047 0.974 (2071 / 2127), far2048 0.881
# (2071 / 2353), far65535 1.000 (65844 / 65844), random_x2 1.000 (131081 /
# 131081), real_page 0.918 (466 / 508).
PINS = {"zeros": 1.0, "random": 1.0, "one_byte": 1.0, "period2": 1.0, "x16": 1.1, "skewed": 1.0, "far2047": 1.0,
        "far2048": 0.9, "far65535": 1.0, "random_x2": 1.0, "real_page": 1.0}
