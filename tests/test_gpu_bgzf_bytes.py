"""The device BGZF inflate (bgzf_inflate.hip: the token pass and the resolve
pass, through bqsr_bgzf_inflate -- the code bqsr_bam_parse's device form
runs, with no host form behind it) against zlib, byte for byte, on crafted
DEFLATE: the members of _bgzf_cases.py, written bit by bit (_deflate.py) so
that they take the decoder's every path -- forms zlib never writes for
SAM-like data among them -- and malformed members, which the decoder must
decline (a non-zero status; which one is not asserted, zlib has no such
classes) without disturbing the members around them.  Integer data: no
tolerance anywhere.  test_deflate_writer.py holds the same members against
zlib on the CPU, so zlib decides both the bytes and accept / reject.

A group of members is one BGZF buffer and one call.  No valid member is
declined: the decoder's second-level distance table (256 entries, root 8)
holds every complete code of at most 30 symbols (the largest needs 144, by
enumeration of all 4.3 million of them), so DIST30 -- 134 -- inflates on the
device like the rest."""
import zlib

import numpy as np
import pytest

import _bgzf_cases as C
import _deflate as D
from adam_amd import bqsr
from adam_amd.sam import bgzf_inflate

pytestmark = pytest.mark.gpu


def _check(members, buf):
    """One call over the buffer; every member against zlib."""
    out, status = bgzf_inflate(buf)
    lay = D.layout(buf)
    assert len(status) == len(lay) >= len(members)
    assert len(out) == sum(l[3] for l in lay)
    wrong = []
    for i, (m, (src, csize, dst, isize)) in enumerate(zip(members, lay)):
        if m.good:
            want = np.frombuffer(zlib.decompress(buf[src:src + csize], -15), np.uint8)
            assert len(want) == isize
            if status[i] != 0:
                wrong.append("%s: declined (status %d)" % (m.name, status[i]))
            elif not np.array_equal(out[dst:dst + isize], want):
                wrong.append("%s: %d bytes differ, the first at %d" % (
                    m.name, int((out[dst:dst + isize] != want).sum()), int(np.argmax(out[dst:dst + isize] != want))))
        elif status[i] == 0:
            wrong.append("%s: accepted" % m.name)
    assert not wrong, wrong
    assert not status[len(members):].any()  # (the EOF block)
    return out, status


@pytest.mark.parametrize("name", sorted(C.GROUPS))
def test_crafted_members(name):
    members = C.GROUPS[name]()
    _check(members, C.pack(members, eof=name in ("codes", "invalid")))


def test_size_query_and_empty_input():
    import ctypes
    from adam_amd import _capi
    from adam_amd.sam import _lib
    L = _lib()
    ctx = bqsr.Context.get(0)
    members = C.group_resolve()
    buf = C.pack(members)
    n, nb = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert L.bqsr_bgzf_inflate(ctx.handle, buf, len(buf), None, None, 0, ctypes.byref(n), None, 0, ctypes.byref(nb)) == 0
    assert n.value == sum(len(m.data) for m in members) and nb.value == len(members)
    out = np.zeros(n.value, np.uint8)
    st = np.zeros(nb.value, np.int32)
    # a buffer too small is refused, not overrun
    assert L.bqsr_bgzf_inflate(ctx.handle, buf, len(buf), None, out.ctypes.data, n.value - 1, ctypes.byref(n),
                               st.ctypes.data, nb.value, ctypes.byref(nb)) == _capi.INVALID_ARG
    assert L.bqsr_bgzf_inflate(ctx.handle, buf, len(buf), None, out.ctypes.data, n.value, ctypes.byref(n),
                               st.ctypes.data, nb.value - 1, ctypes.byref(nb)) == _capi.INVALID_ARG
    assert L.bqsr_bgzf_inflate(ctx.handle, buf[:-1], len(buf) - 1, None, None, 0, ctypes.byref(n), None, 0,
                               ctypes.byref(nb)) == _capi.SAM_PARSE
    out, status = bgzf_inflate(b"")
    assert len(out) == 0 and len(status) == 0


def test_crafted_members_a_block_a_run(monkeypatch):
    # the symbol buffer reused over runs of one block each (ADAM_BQSR_BGZF_RUN)
    members = C.group_codes() + C.group_invalid() + C.group_resolve()
    buf = C.pack(members)
    want = _check(members, buf)
    monkeypatch.setenv("ADAM_BQSR_BGZF_RUN", "1")
    got = _check(members, buf)
    good = np.array([m.good for m in members])
    assert np.array_equal(got[1][good], want[1][good]) and np.all(got[1][~good] != 0)


def test_crafted_members_among_many():
    # more members than the device holds at once at 16 a workgroup (n_cu * 32): the 12-a-workgroup
    # instantiation of the token pass, on one-byte members with the crafted ones spread among them
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    crafted = C.group_codes() + C.group_blocks()[:8] + C.group_invalid()
    ones = [C.fix("one-%d" % i, [i % 251]) for i in range(251)]
    members, k = [], 0
    step = (n_cu * 32 + 300) // len(crafted) + 1
    for c in crafted:
        members += [ones[(k + i) % 251] for i in range(step)] + [c]
        k += step
    assert len(members) > n_cu * 32 + 256
    _check(members, C.pack(members))
