"""BAM output encoded on the device (adam_amd/csrc/bam_out.hip:
bqsr_sam_bam_prepare / _records / _header, bqsr_bgzf_compress, transform's
_BamOut sink) against tests/_bam_ref.py, the encoder written from the SAM
spec, and through the project's own BAM ingest."""
import os

import pytest

import _bam_ref as B
from adam_amd import _capi, synth
from adam_amd.bam_writer import sam_to_bam
from adam_amd.sam import BGZF_EOF, SamText, bgzf_compress
from adam_amd.samgen import sam_text
from adam_amd.transform import main, transform

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "reference_resources")
FIXTURES = ["artificial.realigned.sam", "artificial.sam", "reads12.sam", "small.sam",
            "small_realignment_targets.sam", "unmapped.sam"]
COLS = ["flags", "rg_id", "ref_index", "start", "seq_offset", "seq", "qual_offset", "qual", "cigar_offset", "cigar",
        "md_offset", "md"]

HEAD = (b"@HD\tVN:1.4\tSO:unsorted\n@SQ\tSN:chr1\tLN:1000000\n@SQ\tSN:chr2\tLN:2000000\n"
        b"@RG\tID:g1\tLB:l1\tSM:s\n@RG\tID:g2\tLB:l2\tSM:s\n")

INTS = [-129, -128, 127, 128, 255, 256, -32769, -32768, 32767, 32768, 65535, 65536, 2 ** 31 - 1, 2 ** 31,
        2 ** 32 - 1, -2 ** 31]
SEQ101 = (b"acgtnACGTN=MRSVWYHKDBmrsvwyhkdb.XZ" * 3)[:101]
B_TAGS = [b"BA:B:c", b"BB:B:c,-128,127", b"BC:B:C,0,255", b"BD:B:s,-32768,32767", b"BE:B:S,0,65535",
          b"BF:B:i,-2147483648,2147483647", b"BG:B:I,0,4294967295", b"BH:B:f,1.5,-0.25,0.1"]


def rec(qname=b"r", flag=0, rname=b"chr1", pos=100, mapq=30, cigar=b"*", rnext=b"*", pnext=0, tlen=0, seq=b"*",
        qual=b"*", tags=()):
    return b"\t".join([qname, b"%d" % flag, rname, b"%d" % pos, b"%d" % mapq, cigar, rnext, b"%d" % pnext,
                       b"%d" % tlen, seq, qual] + list(tags)) + b"\n"


def crafted(with_b: bool = True) -> bytes:
    q101 = bytes(33 + (i * 7) % 94 for i in range(101))
    lines = [
        rec(b"ints", 99, b"chr1", 1000, 60, b"2M", b"=", 1200, 202, b"AC", b"I~",
            [b"X%X:i:%d" % (k, v) for k, v in enumerate(INTS)] + [b"RG:Z:g1"]),
        rec(b"floats", 16, b"chr2", 5, 0, b"1M", b"chr1", 7, -3, b"g", b"!",
            [b"FA:f:1.5", b"FB:f:0.1", b"FC:f:1e-10", b"FD:f:3.4028235e38", b"FE:f:-0.0"]),
        rec(b"misc", 0, b"chr1", 20000, 3, b"50M1D20M3I28M", b"*", 0, 0, SEQ101, q101,
            [b"XA:A:Q", b"XZ:Z:", b"XH:H:1AE301", b"RG:Z:g2", b"MD:Z:50^A48"]),
        rec(b"q", 4, b"*", 0, 0, b"*", b"*", 0, 0, b"*", b"*"),                   # "*" SEQ / QUAL / CIGAR
        rec(b"n" * 254, 4, b"*", 0, 0, b"*", b"*", 0, 0, b"ACGTA", b"*"),           # QUAL "*" with a SEQ: 0xFF bytes
        rec(b"pos0", 0, b"chr1", 0, 0, b"3M", b"=", 0, 0, b"NNN", b"###"),         # POS 0: pos -1, bin 4680
        rec(b"far", 163, b"chr2", 1 << 20, 255, b"10M70000N10M", b"chr2", 1 << 21, 80000, b"ACGTACGTACGTACGTACGT",
            b"I" * 20, [b"NM:i:0"]),                                                # a span across bin levels
    ]
    if with_b:
        lines.append(rec(b"arrays", 0, b"chr1", 77, 1, b"4M", b"*", 0, 0, b"ACGT", b"IIII", B_TAGS))
    return HEAD + b"".join(lines)


def simple(n: int, length: int = 100, seed: int = 3) -> bytes:
    """n mapped reads of about `length` bases with a few tags"""
    out = [HEAD]
    for i in range(n):
        L = length + (i * seed) % 7 - 3
        s = bytes(b"ACGT"[(i + j * j) & 3] for j in range(L))
        q = bytes(33 + (i + 5 * j) % 60 for j in range(L))
        out.append(rec(b"s%d" % i, 16 * (i & 1), b"chr%d" % (1 + i % 2), 1 + 997 * i, i % 61, b"%dM" % L, b"=",
                       1 + 997 * i + 200, 300, s, q, [b"NM:i:%d" % (i % 300), b"RG:Z:g%d" % (1 + i % 2)]))
    return b"".join(out)


def file_stream(data: bytes) -> bytes:
    """a BAM file's inflated stream, every member checked (BC field, BSIZE,
    CRC32, ISIZE <= 65280), no empty member but the final EOF marker"""
    assert data.endswith(BGZF_EOF)
    members = B.bgzf_members(data)
    assert members[-1] == (b"", 28)
    assert all(0 < len(raw) <= 65280 for raw, _ in members[:-1])
    return b"".join(raw for raw, _ in members)


def encode(text: bytes, level: int = 6) -> bytes:
    """header + records of a SAM text as a BAM file, by the library"""
    s = SamText(text)
    try:
        head, recs = s.bam_header(), s.bam_records()
        assert len(head) + len(recs) == len(B.stream(text))
        return bgzf_compress(head + recs.tobytes(), level) + BGZF_EOF
    finally:
        s.close()


def ingest(bam: bytes):
    s = SamText(bam, bam=True)
    try:
        return s.text(), s.batch()
    finally:
        s.close()


def assert_same_parse(a: bytes, b: bytes):
    (ta, ba), (tb, bb) = ingest(a), ingest(b)
    assert ta == tb
    assert ba.n_reads == bb.n_reads and ba.ref_names == bb.ref_names
    for c in COLS:
        x, y = getattr(ba, c), getattr(bb, c)
        assert x.dtype == y.dtype and (x == y).all(), c


# ---- 1. stream equality with the spec encoder ----

def test_crafted_stream_equals_reference():
    text = crafted()
    got = file_stream(encode(text))
    want = B.stream(text)
    if got != want:  # name the first record that differs
        h = len(B.header(text)[0])
        assert got[:h] == want[:h], "header"
        for i, (x, y) in enumerate(zip(B.parse_stream(got)[2], B.parse_stream(want)[2])):
            assert x == y, "record %d" % i
    assert got == want


# ---- 2. shapes ----

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_wave_tails(n):
    text = simple(n)
    assert file_stream(encode(text)) == B.stream(text)


@pytest.fixture(scope="module")
def many():
    text = simple(1025)
    return text, B.header(text)[0], B.records(text)


def test_more_than_one_workgroup_records_straddle_members(many):
    text, head, recs = many
    data = encode(text)
    assert file_stream(data) == head + b"".join(recs)
    members = B.bgzf_members(data)
    assert len(members) >= 5  # several 65280-byte members, so records straddle them
    bounds, at = set(), len(head)
    for r in recs:
        at += len(r)
        bounds.add(at)
    assert any(k * 65280 not in bounds for k in range(1, len(members) - 1))


@pytest.mark.parametrize("r0,n", [(3, 70), (60, 10), (63, 1), (64, 64), (1000, 25), (5, 0), (0, 1025)])
def test_sub_ranges(many, r0, n):
    text, _, recs = many
    s = SamText(text)
    try:
        assert s.bam_records(r0, n).tobytes() == b"".join(recs[r0:r0 + n])
    finally:
        s.close()


def test_stream_of_exactly_two_members():
    base = simple(600)
    pad = 2 * 65280 - len(B.stream(base + rec(b"pad", 4, b"*", 0, 0, tags=[b"XP:Z:"])))
    assert 0 < pad < 65280
    text = base + rec(b"pad", 4, b"*", 0, 0, tags=[b"XP:Z:" + b"p" * pad])
    assert len(B.stream(text)) == 2 * 65280
    data = encode(text)
    assert file_stream(data) == B.stream(text)
    assert [len(raw) for raw, _ in B.bgzf_members(data)] == [65280, 65280, 0]  # no empty trailing member


def test_long_cigar_and_many_tags():
    seq = b"ACGT" * 75
    text = HEAD + rec(b"a", 0, b"chr1", 5, 9, b"2M", seq=b"AC", qual=b"II") + \
        rec(b"cig", 0, b"chr2", 3000, 9, b"1M1I" * 150, seq=seq, qual=b"5" * 300) + \
        rec(b"tags", 0, b"chr1", 9, 9, b"1M", seq=b"A", qual=b"I",
            tags=[b"%c%c:i:%d" % (65 + k // 26, 65 + k % 26, k * 1000 - 7) for k in range(40)])
    got = file_stream(encode(text))
    assert got == B.stream(text)
    recs = B.parse_stream(got)[2]
    assert len(recs[1]["cigar"]) == 300


# ---- 3. round trip through the project's own ingest ----

@pytest.mark.parametrize("name", FIXTURES)
def test_round_trip_fixtures(name):
    with open(os.path.join(GOLD, name), "rb") as fh:
        text = fh.read()
    assert_same_parse(encode(text), sam_to_bam(text))


def test_round_trip_crafted():
    text = crafted(with_b=False)
    assert_same_parse(encode(text), sam_to_bam(text))
    # bam_writer cannot write B arrays: the ingest prints them back as they went in
    back, _ = ingest(encode(crafted()))
    line = [l for l in back.split(b"\n") if l.startswith(b"arrays\t")][0]
    assert line.split(b"\t")[11:] == B_TAGS


# ---- 4. transform end to end ----

def bam_text(path) -> bytes:
    with open(path, "rb") as fh:
        data = fh.read()
    file_stream(data)
    return ingest(data)[0]


def sam_of(tmp_path, name: str, text: bytes) -> str:
    p = tmp_path / name
    p.write_bytes(text)
    return str(p)


@pytest.fixture(scope="module")
def gen2000():
    return sam_text(synth.generate(2000, lens=(100,), n_rg=2, seed=11, p_q2tail=0.0), n_rg=2)


def fixture_text() -> bytes:
    with open(os.path.join(GOLD, "small_realignment_targets.sam"), "rb") as fh:
        return fh.read()


@pytest.mark.parametrize("which", ["fixture", "gen"])
@pytest.mark.parametrize("bam_in", [False, True])
def test_transform_markdup_sort(tmp_path, gen2000, which, bam_in):
    text = fixture_text() if which == "fixture" else gen2000
    inp = sam_of(tmp_path, "in.bam" if bam_in else "in.sam", sam_to_bam(text) if bam_in else text)
    xb, xs = str(tmp_path / "X.bam"), str(tmp_path / "X.sam")
    st = transform(inp, xb, mark_duplicates=True, sort_reads=True)
    transform(inp, xs, mark_duplicates=True, sort_reads=True)
    assert st["bam"]["record_bytes"] > 0 and not os.path.exists(xb + ".partial")
    with open(xs, "rb") as fh:
        assert bam_text(xb) == fh.read()


def test_transform_partitions(tmp_path, gen2000):
    inp = sam_of(tmp_path, "in.sam", gen2000)
    xb, xs = str(tmp_path / "X.bam"), str(tmp_path / "X.sam")
    st = transform(inp, xb, mark_duplicates=True, partition_bytes=len(gen2000) // 4)
    transform(inp, xs, mark_duplicates=True, partition_bytes=len(gen2000) // 4)
    assert st["partitions"] >= 3
    with open(xs, "rb") as fh:
        assert bam_text(xb) == fh.read()


def test_transform_pieces_and_level_0(tmp_path, gen2000):
    """stored members, through the CLI; and several pieces per emit"""
    inp = sam_of(tmp_path, "in.sam", gen2000)
    xb, xs, xp = str(tmp_path / "X.bam"), str(tmp_path / "X.sam"), str(tmp_path / "P.bam")
    assert main([inp, xb, "-mark_duplicate_reads", "-sort_reads", "-bam_compression_level", "0"]) == 0
    transform(inp, xs, mark_duplicates=True, sort_reads=True)
    with open(xb, "rb") as fh:
        data = fh.read()
    assert all(size == len(raw) + 31 for raw, size in B.bgzf_members(data)[:-1])
    with open(xs, "rb") as fh:
        want = fh.read()
    assert bam_text(xb) == want
    transform(inp, xp, mark_duplicates=True, sort_reads=True, bam_piece_reads=300)  # 7 pieces, mid-wave cuts
    assert bam_text(xp) == want
    with open(xp, "rb") as fh:
        assert file_stream(fh.read()) == file_stream(data)


def bam_holds(line: bytes) -> bool:
    f = line.split(b"\t")
    return f[10] == b"*" or (len(f[10]) == (0 if f[9] == b"*" else len(f[9])) and all(33 <= c <= 126 for c in f[10]))


def test_transform_recalibrate(tmp_path):
    # a generator seed at which no recalibrated char leaves '!'..'~' (a table of 2 000 reads is sparse: at
    # other seeds a few bins give newP > 1, a char below '!', quirk Q14); asserted on the SAM output below
    gen = sam_text(synth.generate(2000, lens=(100,), n_rg=2, seed=15, p_q2tail=0.0), n_rg=2)
    inp = sam_of(tmp_path, "in.sam", gen)
    xb, xs = str(tmp_path / "X.bam"), str(tmp_path / "X.sam")
    transform(inp, xs, recalibrate=True)
    with open(xs, "rb") as fh:
        want = fh.read()
    lines = [l for l in want.split(b"\n") if l and not l.startswith(b"@")]
    # the precondition: no trimmed string, no char outside '!'..'~', and the quals did change
    assert len(lines) == 2000 and all(bam_holds(l) for l in lines)
    before = [l.split(b"\t")[10] for l in gen.split(b"\n") if l and not l.startswith(b"@")]
    assert sum(l.split(b"\t")[10] != q for l, q in zip(lines, before)) > 0
    transform(inp, xb, recalibrate=True)
    assert bam_text(xb) == want


def test_transform_q2_tail_is_refused(tmp_path):
    text = sam_text(synth.generate(2000, lens=(100,), n_rg=2, seed=11, p_q2tail=0.2), n_rg=2)
    inp = sam_of(tmp_path, "in.sam", text)
    xb, xs = str(tmp_path / "X.bam"), str(tmp_path / "X.sam")
    transform(inp, xs, recalibrate=True)
    with open(xs, "rb") as fh:
        lines = [l for l in fh.read().split(b"\n") if l and not l.startswith(b"@")]
    bad = [i for i, l in enumerate(lines) if not bam_holds(l)]
    assert bad, "the input gives no string BAM cannot hold"
    with pytest.raises(_capi.BQSRError) as e:
        transform(inp, xb, recalibrate=True)
    assert e.value.status == _capi.UNSUPPORTED and e.value.read == bad[0]
    assert "QUAL" in str(e.value) and "SAM text sink" in str(e.value)
    assert not os.path.exists(xb) and not os.path.exists(xb + ".partial")


# ---- 5. refusals ----

LONG_CIGAR = rec(b"c", 0, b"chr1", 1, 0, b"1M" * 65536, seq=b"A" * 65536, qual=b"*")
REFUSALS = {
    "rname": rec(rname=b"chrX"),
    "rnext": rec(rnext=b"chrX"),
    "qname255": rec(qname=b"n" * 255),
    "cigar65536": LONG_CIGAR,
    "pos": rec(pos=2 ** 31 + 1),
    "pos_low": rec(pos=-2 ** 31),
    "pnext": rec(pnext=2 ** 31 + 1),
    "tlen_high": rec(tlen=2 ** 31),
    "tlen_low": rec(tlen=-2 ** 31 - 1),
    "qual_short": rec(cigar=b"3M", seq=b"ACG", qual=b"II"),          # a trimmed string (quirk Q13)
    "qual_long": rec(cigar=b"3M", seq=b"ACG", qual=b"IIII"),
    "qual_no_seq": rec(seq=b"*", qual=b"I"),
    "qual_space": rec(cigar=b"3M", seq=b"ACG", qual=b"I I"),
    "qual_del": rec(cigar=b"3M", seq=b"ACG", qual=b"I\x7fI"),
    "qual_utf8": rec(cigar=b"3M", seq=b"ACG", qual=b"I\xc2\x80"),    # a char above 0x7F (quirk Q14), UTF-8
    "tag_type": rec(tags=[b"XX:Q:1"]),
    "array_type": rec(tags=[b"XX:B:x,1"]),
    "int_high": rec(tags=[b"XX:i:4294967296"]),
    "int_low": rec(tags=[b"XX:i:-2147483649"]),
    "int_huge": rec(tags=[b"XX:i:123456789012345678901234567890"]),
    "B_c": rec(tags=[b"XX:B:c,0,128"]),
    "B_C": rec(tags=[b"XX:B:C,-1"]),
    "B_s": rec(tags=[b"XX:B:s,32768"]),
    "B_S": rec(tags=[b"XX:B:S,65536"]),
    "B_i": rec(tags=[b"XX:B:i,2147483648"]),
    "B_I": rec(tags=[b"XX:B:I,4294967296"]),
    "B_I_neg": rec(tags=[b"XX:B:I,-1"]),
    "H_odd": rec(tags=[b"XX:H:ABC"]),
    "H_nonhex": rec(tags=[b"XX:H:AG"]),
}
GOOD = rec(b"ok", 0, b"chr1", 10, 20, b"4M", b"=", 30, 24, b"ACGT", b"IIII", [b"NM:i:1", b"XF:f:2.5"])


def refused(text: bytes, r0: int = 0, n=None) -> int:
    s = SamText(text)
    try:
        with pytest.raises(_capi.BQSRError) as e:
            s.bam_records(r0, n)
        assert e.value.status == _capi.UNSUPPORTED
        return e.value.read
    finally:
        s.close()


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusal_names_the_read(name):
    text = HEAD + GOOD + REFUSALS[name] + GOOD
    with pytest.raises(B.BamRefusal) as e:
        B.records(text)
    assert e.value.read == 1
    assert refused(text) == 1


def test_earlier_refusal_wins():
    lines = [GOOD] * 200
    lines[150] = REFUSALS["rname"]
    lines[70] = REFUSALS["H_odd"]
    text = HEAD + b"".join(lines)
    assert refused(text) == 70
    assert refused(text, 71, 100) == 150  # a sub-range past the first: the read's index in the parse
    s = SamText(text)
    try:
        assert s.bam_records(0, 70).tobytes() == b"".join(B.records(HEAD + GOOD * 70))
    finally:
        s.close()


# ---- 6. the sink's contract ----

def test_existing_output_needs_overwrite(tmp_path):
    inp = sam_of(tmp_path, "in.sam", simple(10))
    xb = str(tmp_path / "X.bam")
    transform(inp, xb)
    with open(xb, "rb") as fh:
        first = fh.read()
    assert file_stream(first) == B.stream(simple(10))
    with pytest.raises(FileExistsError):
        transform(inp, xb)
    with open(xb, "rb") as fh:
        assert fh.read() == first
    transform(inp, xb, overwrite=True)
    with open(xb, "rb") as fh:
        assert file_stream(fh.read()) == file_stream(first)


def test_partial_is_removed_after_a_failure(tmp_path):
    inp = sam_of(tmp_path, "in.sam", HEAD + GOOD * 5 + REFUSALS["rnext"] + GOOD)
    xb = str(tmp_path / "X.bam")
    with pytest.raises(_capi.BQSRError) as e:
        transform(inp, xb, bam_piece_reads=2)  # pieces were appended before the refusal
    assert e.value.read == 5
    assert not os.path.exists(xb) and not os.path.exists(xb + ".partial")


def test_parquet_input_is_refused(tmp_path):
    with pytest.raises(ValueError, match="BAM"):
        transform(str(tmp_path / "reads.adam"), str(tmp_path / "X.bam"))
    assert os.listdir(str(tmp_path)) == []
