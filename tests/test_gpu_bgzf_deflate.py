"""BGZF members deflated on the device (adam_amd/csrc/bgzf_deflate.hip through
bqsr_bgzf_deflate) against an independent decoder: every member's frame, its
body inflated on its own by zlib, CRC32 and ISIZE; the same bytes from two
runs, from the project's device inflate and from the member routine compiled
for the host; the derived size conditions; one regression pin."""
import ctypes
import os

import numpy as np
import pytest

import _bam_ref as B
import _deflate_cases as C
from adam_amd import _capi, bqsr
from adam_amd.sam import _lib, bgzf_deflate, bgzf_deflate_host, bgzf_inflate

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "reference_resources")


def check(data: bytes):
    """every member of the device's output for `data`; returns [(raw, size)]"""
    out = bgzf_deflate(data)
    ms = C.check_members(out, data)
    assert bgzf_deflate(data) == out, "two runs differ"
    assert bgzf_deflate_host(data) == out, "the host-compiled routine differs"
    if data:
        back, status = bgzf_inflate(out)
        assert len(status) == len(ms) and (status == 0).all()
        assert back.tobytes() == data
    else:
        assert out == b""
    return ms


@pytest.mark.parametrize("kind", ["random", "zeros"])
@pytest.mark.parametrize("n", C.SIZES)
def test_sizes(n, kind):
    ms = check(C.random_bytes(n, 100 + n) if kind == "random" else bytes(n))
    assert [len(raw) for raw, _ in ms] == [C.MEMBER] * (n // C.MEMBER) + ([n % C.MEMBER] if n % C.MEMBER else [])


@pytest.mark.parametrize("name", C.CONTENTS)
def test_contents(name):
    ms = check(C.content(name))
    assert len(ms) == (2 if name == "T" else 1)
    C.check_sizes(name, ms)


def test_more_members_than_workgroups():
    """a grid that loops: more members than the device has CUs, their contents differing"""
    rng = np.random.default_rng(11)
    n = 300 * C.MEMBER + 1234
    data = (rng.integers(0, 4, n, dtype=np.uint8) * rng.integers(0, 2, n, dtype=np.uint8) + 65).tobytes()
    out = bgzf_deflate(data)
    ms = C.check_members(out, data)
    assert len(ms) == 301 and len(out) < n // 2


def test_output_that_does_not_fit():
    L, ctx = _lib(), bqsr.Context.get(0)
    data = np.frombuffer(C.content("A") + C.content("B"), np.uint8)
    want = bgzf_deflate(data)
    out = np.zeros(len(want), np.uint8)
    got, nm = ctypes.c_int64(), ctypes.c_int64()
    rc = L.bqsr_bgzf_deflate(ctx.handle, data.ctypes.data, data.size, None, out.ctypes.data, len(want) - 1,
                             ctypes.byref(got), ctypes.byref(nm))
    assert rc == _capi.INVALID_ARG and got.value == len(want) and nm.value == 2
    assert L.bqsr_bgzf_deflate(ctx.handle, data.ctypes.data, data.size, None, out.ctypes.data, len(want),
                               ctypes.byref(got), ctypes.byref(nm)) == 0
    assert out.tobytes() == want
    assert len(want) <= data.size + 64 * (data.size // 65280 + 1)


# Device size / zlib level-1 size, measured on the first run of this kernel and
# rounded up to one decimal (the output is a function of the input alone, so
# the figure moves only when the kernel or zlib's level 1 does): A 1.025 (4883
# / 4765 bytes), B 0.947 (31796 / 33567), F 0.972 (19429 / 19981), Z 0.262 (79
# / 302), the record stream of small_realignment_targets.sam 1.016 (1069 /
# 1052).
PINS = {"A": 1.1, "B": 1.0, "F": 1.0, "Z": 0.3, "records": 1.1}


@pytest.mark.parametrize("name", sorted(PINS))
def test_size_pin(name):
    if name == "records":
        with open(os.path.join(GOLD, "small_realignment_targets.sam"), "rb") as fh:
            text = fh.read()
        data = b"".join(B.records(text))
    else:
        data = C.content(name)
    ms = C.check_members(bgzf_deflate(data), data)
    ratio = C.body_size(ms) / sum(C.zsize(raw, 1) for raw, _ in ms)
    print("size pin %s: device %d bytes, zlib level 1 %d, ratio %.4f" % (
        name, C.body_size(ms), sum(C.zsize(raw, 1) for raw, _ in ms), ratio))
    assert ratio <= PINS[name]
