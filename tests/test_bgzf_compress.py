"""bqsr_bgzf_compress (host threads, no device): every member carries the BC
field with its BSIZE, CRC32 and ISIZE <= 65280, the members inflate to the
input, no empty member and no EOF marker is written, level 0 is stored."""
import numpy as np
import pytest

import _bam_ref as B
from adam_amd.sam import BGZF_EOF, bgzf_compress


def data_of(n: int, kind: str) -> bytes:
    if kind == "random":  # incompressible: the stored fallback must still fit BSIZE
        return np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    return (b"ACGTTGCA" * (n // 8 + 1))[:n]


@pytest.mark.parametrize("level", [0, 1, 6, 9])
@pytest.mark.parametrize("n", [0, 1, 65279, 65280, 65281, 2 * 65280, 5 * 65280 + 17])
@pytest.mark.parametrize("kind", ["text", "random"])
def test_members(n, level, kind):
    data = data_of(n, kind)
    out = bgzf_compress(data, level)
    members = B.bgzf_members(out)  # checks BC / BSIZE, CRC32, ISIZE
    assert len(members) == (n + 65279) // 65280
    assert all(0 < len(raw) <= 65280 for raw, _ in members)
    assert all(len(raw) == 65280 for raw, _ in members[:-1])
    assert b"".join(raw for raw, _ in members) == data
    assert all(size <= 65536 for _, size in members)
    if level == 0:  # stored: 18 + 5 + the bytes + 8
        assert all(size == len(raw) + 31 for raw, size in members)
    elif kind == "text" and n > 1000:
        assert len(out) < n // 4
    # a file: the members, then the marker
    assert B.bgzf_members(out + BGZF_EOF)[-1] == (b"", 28)


def test_bad_level():
    from adam_amd._capi import BQSRError
    with pytest.raises(BQSRError):
        bgzf_compress(b"abc", 10)
