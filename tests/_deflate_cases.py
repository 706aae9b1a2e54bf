"""Inputs and checks shared by the device DEFLATE tests (bgzf_deflate.hip):
test_deflate_codes.py runs them through the member routine compiled for the
host (sam.bgzf_deflate_host), test_gpu_bgzf_deflate.py through the device.

The oracle for a compressor is an independent decoder: every member's body is
inflated by a fresh ``zlib.decompressobj(-15)``, so a reference across members
fails.  The size conditions compare with zlib on the same member, computed
here."""
import struct
import zlib

import numpy as np

from _deflate import layout

MEMBER = 65280
HEAD = bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0]) + b"BC" + struct.pack("<H", 2)

SIZES = [0, 1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 258, 259, 260, 65279, 65280, 65281, 130560, 130561]

FIB22 = [1, 1]
while len(FIB22) < 22:
    FIB22.append(FIB22[-1] + FIB22[-2])
assert sum(FIB22) == 46367


def random_bytes(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _far(dist: int) -> bytes:
    x = random_bytes(300, 21)
    return x + random_bytes(dist - 300, 22) + x


def content(name: str) -> bytes:
    if name == "Z":
        return bytes(MEMBER)
    if name == "R":
        return random_bytes(MEMBER, 5)
    if name == "A":
        return random_bytes(4080, 6) * 16
    if name == "B":
        p = 0.75 ** np.arange(64)
        return np.random.default_rng(7).choice(64, MEMBER, p=p / p.sum()).astype(np.uint8).tobytes()
    if name == "F":
        a = np.concatenate([np.full(c, i, np.uint8) for i, c in enumerate(FIB22)])
        np.random.default_rng(3).shuffle(a)
        return a.tobytes()
    if name == "S":
        return b"\x41" * MEMBER
    if name == "P":
        return b"\x41\x5a" * (MEMBER // 2)
    if name == "D":
        return _far(32768)
    if name == "D'":
        return _far(32769)
    if name == "T":
        return random_bytes(MEMBER, 8) * 2
    raise KeyError(name)


CONTENTS = ["Z", "R", "A", "B", "F", "S", "P", "D", "D'", "T"]


def members(out: bytes):
    """[(raw, size)] of a buffer of BGZF members, every one checked: header
    bytes, BSIZE, the body inflated on its own to the end of the stream with
    nothing left over, CRC32, ISIZE"""
    res, at = [], 0
    for src, csize, _, isize in layout(out):
        assert out[at:at + 16] == HEAD, "header bytes"
        bsize, = struct.unpack_from("<H", out, at + 16)
        size = bsize + 1
        assert size == 18 + csize + 8 and size <= 65536 and src == at + 18
        d = zlib.decompressobj(-15)
        raw = d.decompress(out[src:src + csize])
        assert d.eof and d.unused_data == b"" and d.unconsumed_tail == b""
        crc, isz = struct.unpack_from("<II", out, src + csize)
        assert isz == isize == len(raw) and crc == zlib.crc32(raw)
        res.append((raw, size))
        at += size
    assert at == len(out)
    return res


def check_members(out: bytes, data: bytes):
    """the frame and the body of every member of `out`, which must hold `data`"""
    ms = members(out)
    assert len(ms) == (len(data) + MEMBER - 1) // MEMBER
    assert all(len(raw) == MEMBER for raw, _ in ms[:-1])
    assert all(0 < len(raw) <= MEMBER for raw, _ in ms)
    assert b"".join(raw for raw, _ in ms) == data
    assert all(size <= len(raw) + 31 for raw, size in ms)  # never above the stored form
    return ms


def zsize(raw: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY) -> int:
    """bytes of raw DEFLATE zlib makes of one member"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return len(c.compress(raw) + c.flush())


def body_size(ms) -> int:
    return sum(size - 26 for _, size in ms)


def check_sizes(name: str, ms):
    """the derived size conditions of the named contents"""
    raw = ms[0][0]
    body = ms[0][1] - 26
    if name in ("A", "Z"):  # matches and runs are used
        assert body < zsize(raw, 6, zlib.Z_HUFFMAN_ONLY)
    if name in ("B", "F"):  # dynamic codes are used
        assert body < zsize(raw, 6, zlib.Z_FIXED)
    if name == "R":  # stored
        assert ms[0][1] == MEMBER + 31
