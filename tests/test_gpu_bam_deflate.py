"""BAM records deflated without leaving the device (SamText.bam_members:
bqsr_sam_bam_prepare / _members) and `transform ... OUT.bam -bam_compressor
device`: the members inflate to exactly what bam_records hands out (float tags
included), and the file holds what the host compressor's file holds."""
import gzip
import os

import pytest

import _bam_ref as B
import _deflate_cases as C
from adam_amd import _capi, synth
from adam_amd.bam_writer import sam_to_bam
from adam_amd.sam import BGZF_EOF, BamSizes, SamText
from adam_amd.samgen import sam_text
from adam_amd.transform import main, transform

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "reference_resources")
FIXTURES = ["artificial.realigned.sam", "artificial.sam", "reads12.sam", "small.sam",
            "small_realignment_targets.sam", "unmapped.sam"]
HEAD = b"@HD\tVN:1.4\tSO:unsorted\n@SQ\tSN:chr1\tLN:1000000\n@SQ\tSN:chr2\tLN:2000000\n@RG\tID:g1\tLB:l1\tSM:s\n"
FLOATS = [b"1.5", b"0.1", b"1e-10", b"3.4028235e38", b"-0.0", b"2.5", b"-7e3", b"0.333333343", b"inf"]


def fixture(name: str) -> bytes:
    with open(os.path.join(GOLD, name), "rb") as fh:
        return fh.read()


def float_sam(n: int = 700) -> bytes:
    """n mapped reads, most with f tags and B:f arrays between other tags: more than one member of records"""
    out = [HEAD]
    for i in range(n):
        L = 90 + i % 21
        seq = bytes(b"ACGT"[(i + j * j) & 3] for j in range(L))
        qual = bytes(33 + (i + 5 * j) % 60 for j in range(L))
        tags = [b"NM:i:%d" % (i % 300)]
        if i % 5:
            tags.append(b"XF:f:" + FLOATS[i % len(FLOATS)])
        if i % 3 == 0:
            tags.append(b"XB:B:f," + b",".join(FLOATS[(i + k) % len(FLOATS)] for k in range(1 + i % 4)))
        if i % 7 == 0:
            tags.append(b"YF:f:%d.%d" % (i, i % 10))
        tags.append(b"RG:Z:g1")
        out.append(b"\t".join([b"f%d" % i, b"%d" % (16 * (i & 1)), b"chr%d" % (1 + i % 2), b"%d" % (1 + 997 * i),
                               b"%d" % (i % 61), b"%dM" % L, b"=", b"%d" % (1 + 997 * i + 200), b"300", seq, qual] +
                              tags) + b"\n")
    return b"".join(out)


def inflated(members: bytes) -> bytes:
    return b"".join(raw for raw, _ in C.members(members))


def check_parse(s: SamText, ranges):
    for r0, n in ranges:
        want = s.bam_records(r0, n).tobytes()
        got = s.bam_members(r0, n)
        assert inflated(got) == want, (r0, n)
        assert len(C.members(got)) == (len(want) + C.MEMBER - 1) // C.MEMBER
        if not want:
            assert got == b""


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures(name):
    s = SamText(fixture(name))
    try:
        n = s.counts().n_reads
        check_parse(s, [(0, None), (1, n - 1), (n // 2, n - n // 2), (n - 1, 1), (0, 0), (n, 0)])
    finally:
        s.close()


def test_bam_born_parse():
    s = SamText(sam_to_bam(fixture("small_realignment_targets.sam")), bam=True)
    try:
        assert s.bam_form != 0
        n = s.counts().n_reads
        check_parse(s, [(0, None), (1, n - 1), (n // 2, 1), (2, 0)])
    finally:
        s.close()


def test_float_tags_and_arrays():
    text = float_sam()
    recs = B.records(text)  # the encoder written from the spec: correctly rounded binary32 values
    s = SamText(text)
    try:
        got = s.bam_members()
        assert inflated(got) == b"".join(recs) == s.bam_records().tobytes()
        assert len(C.members(got)) >= 3  # patches land in every member
        for r0, n in ((1, 699), (64, 65), (500, 200), (699, 1), (10, 0)):
            assert inflated(s.bam_members(r0, n)) == b"".join(recs[r0:r0 + n]), (r0, n)
    finally:
        s.close()


def test_members_after_rewrite_need_a_new_prepare():
    s = SamText(float_sam(50))
    try:
        sz = BamSizes()
        import ctypes
        _capi.check(s.L.bqsr_sam_bam_prepare(s.ctx.handle, s.h, 0, 50, None, ctypes.byref(sz)))
        s.rewrite(None)
        with pytest.raises(_capi.BQSRError) as e:
            s._members(sz.bytes)
        assert e.value.status == _capi.INVALID_ARG and "text changed" in str(e.value)
        assert inflated(s.bam_members()) == s.bam_records().tobytes()
    finally:
        s.close()


# ---- transform ----

@pytest.fixture(scope="module")
def gen2000():
    return sam_text(synth.generate(2000, lens=(100,), n_rg=2, seed=11, p_q2tail=0.0), n_rg=2)


def read(path) -> bytes:
    with open(path, "rb") as fh:
        return fh.read()


@pytest.mark.parametrize("steps", [False, True])
@pytest.mark.parametrize("which", ["fixture", "gen", "floats"])
def test_transform_device_compressor(tmp_path, gen2000, which, steps):
    text = {"fixture": fixture("small_realignment_targets.sam"), "gen": gen2000, "floats": float_sam()}[which]
    inp = str(tmp_path / "in.sam")
    with open(inp, "wb") as fh:
        fh.write(text)
    xd, xh = str(tmp_path / "D.bam"), str(tmp_path / "H.bam")
    flags = ["-sort_reads", "-mark_duplicate_reads"] if steps else []
    assert main([inp, xd, "-bam_compressor", "device"] + flags) == 0
    assert main([inp, xh, "-bam_compressor", "host"] + flags) == 0
    dev, host = read(xd), read(xh)
    assert gzip.decompress(dev) == gzip.decompress(host)
    assert dev[-28:] == BGZF_EOF
    assert not os.path.exists(xd + ".partial")
    members = C.members(dev)
    assert members[-1] == (b"", 28) and all(0 < len(raw) <= C.MEMBER for raw, _ in members[:-1])
    # read back through the project's own BAM ingest: the SAM's flagstat
    a, b = SamText(dev, bam=True), SamText(text)
    try:
        if steps:
            b.mark_duplicates()
        assert a.counts().n_reads == b.counts().n_reads
        assert a.flagstat() == b.flagstat()
    finally:
        a.close()
        b.close()


def test_transform_device_pieces_and_stats(tmp_path, gen2000):
    inp = str(tmp_path / "in.sam")
    with open(inp, "wb") as fh:
        fh.write(gen2000)
    xd, xh = str(tmp_path / "D.bam"), str(tmp_path / "H.bam")
    st = transform(inp, xd, mark_duplicates=True, bam_compressor="device", bam_piece_reads=300)  # 7 pieces
    transform(inp, xh, mark_duplicates=True, bam_piece_reads=300)
    assert gzip.decompress(read(xd)) == gzip.decompress(read(xh))
    b = st["bam"]
    assert b["compressor"] == "device" and b["file_bytes"] == os.path.getsize(xd)
    assert 0 < b["downloaded_bytes"] < b["record_bytes"]  # the members, not the stream
    assert b["deflate_ms"] > 0


def test_transform_device_refusal_leaves_nothing(tmp_path):
    good = b"ok\t0\tchr1\t10\t20\t4M\t=\t30\t24\tACGT\tIIII\tNM:i:1\tXF:f:2.5\n"
    bad = b"bad\t0\tchr1\t10\t20\t*\tchrX\t0\t0\t*\t*\n"
    inp = str(tmp_path / "in.sam")
    with open(inp, "wb") as fh:
        fh.write(HEAD + good * 5 + bad + good)
    xd = str(tmp_path / "D.bam")
    with pytest.raises(_capi.BQSRError) as e:
        transform(inp, xd, bam_compressor="device", bam_piece_reads=2)  # pieces were written before the refusal
    assert e.value.status == _capi.UNSUPPORTED and e.value.read == 5
    assert "read 5" in str(e.value)
    assert not os.path.exists(xd) and not os.path.exists(xd + ".partial")
