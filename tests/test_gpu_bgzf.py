"""BGZF inflated on the device (bgzf_inflate.hip, BQSR_TUNE_BGZF 1) against
the host form (libdeflate / zlib threads, BQSR_TUNE_BGZF 0, the default):
the same BAM recompressed with every DEFLATE block form -- stored (level 0),
fixed Huffman codes (Z_FIXED), dynamic codes at levels 1, 6, 9, Huffman-only
and run-length strategies -- and with members of 100 B to 64 KiB (records
spanning several members, members without a record start) parses to the
same columns.  The records' offsets are found on the device and checked as a
chain; a damaged file takes the host form and fails as before
(test_gpu_sam.py::test_bam_ingest_rejects_damaged_bgzf).  Every parse here
also says which form served it (SamText.bam_form): a device form that
declined would otherwise compare the host form with itself.  The decoder's
bytes are held to zlib's in test_gpu_bgzf_bytes.py."""
import os
import struct
import zlib

import pytest

from adam_amd import bqsr
from adam_amd.bam_writer import sam_to_bam
from adam_amd.sam import SamText
from test_gpu_sam import FIXTURES, GOLD, _dup_sam, assert_same_columns

pytestmark = pytest.mark.gpu

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def _inflate(bam: bytes) -> bytes:
    out, p = [], 0
    while p < len(bam):
        xlen = bam[p + 10] | (bam[p + 11] << 8)
        bsize = bam[p + 16] | (bam[p + 17] << 8)
        out.append(zlib.decompress(bam[p + 12 + xlen:p + bsize + 1 - 8], -15))
        p += bsize + 1
    return b"".join(out)


def _reblock(raw: bytes, block: int, level: int, strategy: int) -> bytes:
    out = []
    for i in range(0, len(raw), block):
        chunk = raw[i:i + block]
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        comp = c.compress(chunk) + c.flush()
        bsize = 18 + len(comp) + 8 - 1
        out.append(struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, bsize) + comp +
                   struct.pack("<II", zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk)))
    out.append(EOF_BLOCK)
    return b"".join(out)


def _columns(data: bytes, bgzf: int):
    with bqsr.Context.get(0).tuned(bgzf=bgzf):
        s = SamText(data, bam=True)
        try:
            assert s.bam_form == (2 if bgzf else 1)
            return s.batch()
        finally:
            s.close()


@pytest.fixture(scope="module")
def raw_bam():
    return _inflate(sam_to_bam(_dup_sam(20000, 4243, 30000)))


@pytest.mark.parametrize("block,level,strategy", [
    (65280, 6, zlib.Z_DEFAULT_STRATEGY),
    (65536, 9, zlib.Z_DEFAULT_STRATEGY),
    (65280, 1, zlib.Z_DEFAULT_STRATEGY),
    (65280, 0, zlib.Z_DEFAULT_STRATEGY),   # stored blocks
    (20000, 6, zlib.Z_FIXED),              # fixed Huffman codes
    (65280, 6, zlib.Z_HUFFMAN_ONLY),       # literals only
    (65280, 6, zlib.Z_RLE),                # distance-1 matches
    (1000, 6, zlib.Z_DEFAULT_STRATEGY),    # records across members
    (100, 6, zlib.Z_DEFAULT_STRATEGY),     # members without a record start
])
def test_device_inflate_equals_host(raw_bam, block, level, strategy):
    data = _reblock(raw_bam, block, level, strategy)
    assert_same_columns(_columns(data, 1), _columns(data, 0))


@pytest.mark.parametrize("name", FIXTURES)
def test_device_inflate_reference_fixtures(name):
    with open(os.path.join(GOLD, name), "rb") as fh:
        data = sam_to_bam(fh.read())
    assert_same_columns(_columns(data, 1), _columns(data, 0))


def test_device_inflate_long_records():
    # records longer than a member (4000-base reads, 600-B members): record
    # starts several members apart, most members without one
    from adam_amd import synth
    from adam_amd.samgen import sam_text
    b = synth.generate(300, (4000,), 1, seed=99)
    data = _reblock(_inflate(sam_to_bam(sam_text(b))), 600, 6, zlib.Z_DEFAULT_STRATEGY)
    assert_same_columns(_columns(data, 1), _columns(data, 0))


@pytest.mark.parametrize("run,block", [(150000, 65280), (100000, 20000), (1, 1000)])
def test_device_inflate_in_runs(raw_bam, monkeypatch, run, block):
    # the symbol buffer reused over runs of whole blocks (ADAM_BQSR_BGZF_RUN
    # bytes of output a run; 1: a block a run)
    data = _reblock(raw_bam, block, 6, zlib.Z_DEFAULT_STRATEGY)
    want = _columns(data, 0)
    monkeypatch.setenv("ADAM_BQSR_BGZF_RUN", str(run))
    assert_same_columns(_columns(data, 1), want)


def test_device_inflate_many_blocks(raw_bam):
    # more blocks than the device holds at once at 16 a workgroup (n_cu * 32):
    # the 12-a-workgroup decode (bam_ingest.hip)
    data = _reblock(raw_bam, 250, 6, zlib.Z_DEFAULT_STRATEGY)
    assert len(raw_bam) // 250 > 256 * 32
    assert_same_columns(_columns(data, 1), _columns(data, 0))


def _member(raw: bytes, chunk: bytes) -> bytes:
    bsize = 18 + len(raw) + 8 - 1
    return (struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, bsize) + raw +
            struct.pack("<II", zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk)))


def _reblock_at(raw: bytes, cuts) -> bytes:
    cuts = sorted(set([0, len(raw)] + [c for c in cuts if 0 < c < len(raw)]))
    out = []
    for a, b in zip(cuts, cuts[1:]):
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        out.append(_member(c.compress(raw[a:b]) + c.flush(), raw[a:b]))
    return b"".join(out + [EOF_BLOCK])


def _sam_columns(text: bytes):
    s = SamText(text)
    try:
        assert s.bam_form == 0
        return s.batch()
    finally:
        s.close()


def test_device_inflate_thirty_distance_codes():
    # a member written with all 30 distance codes declared, 9- to 15-bit ones in three root prefixes
    # (_bgzf_cases.DIST30): within the decoder's second-level table, as every complete distance code is, so
    # the device form serves the file
    import _bgzf_cases as C
    text = _dup_sam(300, 11, 30000)
    raw = _inflate(sam_to_bam(text))
    chunk = raw[2000:5000]
    toks = C.lz_tokens(chunk)
    assert any(not isinstance(t, int) for t in toks)
    m = C.dyn("dist30", toks, C.lens_for(toks, nlen=286)[0], C.DIST30)
    assert zlib.decompress(m.raw, -15) == chunk == m.data
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    head = c.compress(raw[:2000]) + c.flush()
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    tail = c.compress(raw[5000:]) + c.flush()
    data = _member(head, raw[:2000]) + _member(m.raw, chunk) + _member(tail, raw[5000:]) + EOF_BLOCK
    assert_same_columns(_columns(data, 1), _sam_columns(text))


def test_device_declines_fake_records_in_qual():
    # one read's QUAL bytes spell two consecutive plausible records (block_size 40, ref 0, pos 0, l_name 4, a
    # NUL-terminated name, every other field 0, 4 spare bytes; all bytes legal qualities), and a member starts
    # exactly at the first: that member's guess is the fake record, whose walk joins the true chain two records
    # on, but the member before it lands on the true next record, not on the guess -- the chain check rejects,
    # the host form serves the file, and the columns are the SAM text's.  (An accepted chain is the true one.)
    fake = struct.pack("<iiiBBHHHiiii", 40, 0, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0) + b"AAA\0" + b"\0\0\0\0"
    assert len(fake) == 44 and max(fake) <= 93
    lines = _dup_sam(300, 12, 30000).split(b"\n")
    k = next(i for i, l in enumerate(lines) if l and not l.startswith(b"@")) + 100
    f = lines[k].split(b"\t")[:11]
    f[5], f[9], f[10] = b"88M", b"ACGT" * 22, bytes(b + 33 for b in fake + fake)
    lines[k] = b"\t".join(f)
    text = b"\n".join(lines)
    raw = _inflate(sam_to_bam(text))
    at = raw.index(fake + fake)
    assert raw.count(fake + fake) == 1
    want = _sam_columns(text)
    every = list(range(3000, len(raw), 3000))
    data = _reblock_at(raw, [c for c in every if not at - 200 < c < at + 200] + [at])
    with bqsr.Context.get(0).tuned(bgzf=1):
        s = SamText(data, bam=True)
        try:
            assert s.bam_form == 1
            assert_same_columns(s.batch(), want)
        finally:
            s.close()
    # a member starting at the true record after them instead: the device form serves the same file
    data = _reblock_at(raw, [c for c in every if not at - 200 < c < at + 200] + [at + 88])
    assert_same_columns(_columns(data, 1), want)
