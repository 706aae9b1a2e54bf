"""Float tag text on the device (samk::java_float_text, samk::java_parse_float,
adam_amd/csrc/sam_ingest.hip) against exact arithmetic (tests/_float_ref.py) on
the patterns and texts of tests/_float_cases.py, through every path that
converts: BAM ingest (binary32 -> text, `f` tags and B:f arrays, both BGZF
forms), `print_tags -count` over SAM and Arrow input (text -> binary32 -> key ->
text), the ADAMRecord `attributes` column, the BAM encoder's stored bits against
the keys of the same records, and BAM -> text -> key -> text.  Every comparison
is on bytes or bits."""
import collections
import functools
import struct

import pytest

import _bam_ref as B
import _float_cases as C
import _float_ref as F
from adam_amd import adam_save as A
from adam_amd import bqsr
from adam_amd.bam_writer import _bam_header, _bgzf
from adam_amd.sam import SamText
from test_gpu_print_tags import arrow_values, table

pytestmark = pytest.mark.gpu

HEAD = [b"@HD\tVN:1.4", b"@SQ\tSN:c\tLN:100"]


def bam_record(i: int, tags: bytes) -> bytes:
    name = b"r%d\0" % i
    rec = struct.pack("<iiBBHHHiiii", 0, 0, len(name), 60, 4680, 1, 0, 1, -1, -1, 0) + name + \
        struct.pack("<I", 1 << 4) + bytes([0x10, 30]) + tags
    assert len(rec) < 65536
    return struct.pack("<i", len(rec)) + rec


def bam_of(tags) -> bytes:
    return _bgzf(_bam_header(HEAD)[0] + b"".join(bam_record(i, t) for i, t in enumerate(tags)))


def sam_of(texts) -> bytes:
    return b"".join(l + b"\n" for l in HEAD) + \
        b"".join(b"q%d\t0\tc\t1\t60\t1M\t*\t0\t0\tA\tI\tXF:f:%s\n" % (i, t) for i, t in enumerate(texts))


def text_of(t: bytes) -> str:
    """the text Float.toString gives the float Float.parseFloat reads"""
    return F.shortest_text(C.parse_bits()[t])


def bits_of_text(s: str) -> int:
    return F.f32_bits_of_decimal(s.encode())


def wanted_values(texts):
    return dict(collections.Counter(("f", text_of(t)) for t in texts))


@functools.lru_cache(maxsize=None)
def sample():
    """about 230 texts of the parse set: every 29th and all the edges"""
    ps = C.parse_set()
    return tuple(ps[::29]) + tuple(ps[7 * len(C.parse_floats()):])


def differing(got, want, what):
    return [(i, what[i] if what else None, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:12]


# ---- binary32 -> text ------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def render_bam() -> bytes:
    rs = C.render_set()
    return bam_of(b"XFf" + struct.pack("<I", rs[r]) + b"XBBf" + struct.pack("<i4096I", 4096, *rs[r + 1:r + 4097])
                  for r in range(0, len(rs), 4097))


@pytest.mark.parametrize("bgzf", [0, 1])
def test_render_through_bam_ingest(bgzf):
    rs, want = C.render_set(), C.render_texts()
    with bqsr.Context.get(0).tuned(bgzf=bgzf):
        s = SamText(render_bam(), bam=True)
        try:
            assert s.bam_form == (2 if bgzf else 1)
            lines = [l for l in s.text().split(b"\n") if l and not l.startswith(b"@")]
        finally:
            s.close()
    assert len(lines) == 16
    got = []
    for l in lines:
        xf, xb = l.split(b"\t")[11:]
        assert xf.startswith(b"XF:f:") and xb.startswith(b"XB:B:f,")
        got += [xf[5:]] + xb[7:].split(b",")
    assert len(got) == len(rs)
    assert not differing(got, [want[b].encode() for b in rs], [hex(b) for b in rs])
    for b, t in C.LONG_POWERS.items():
        assert got[rs.index(b)] == t.encode()


def test_round_trip_on_the_device():
    """binary32 -> text (ingest) -> binary32 -> key -> text (print_tags -count) over BAM input"""
    pats, texts = C.render_structured(), C.render_texts()
    want = dict(collections.Counter(("f", texts[b]) for b in pats))
    assert want[("f", "NaN")] >= 16 and want[("f", "0.0")] == want[("f", "-0.0")] == 1
    s = SamText(bam_of(b"XFf" + struct.pack("<I", b) for b in pats), bam=True)
    try:
        got = s.tag_values("XF")
    finally:
        s.close()
    assert sorted(got) == sorted(want)
    assert got == want


# ---- text -> binary32 -> text ----------------------------------------------------------

def test_parse_then_render_through_print_tags():
    texts = C.parse_set()
    want = wanted_values(texts)
    assert sum(want.values()) == len(texts)
    assert max(want.values()) >= 5 and want[("f", "NaN")] == 3 and want[("f", "1.5")] >= 5  # texts of one float merge
    keys = {bits_of_text(k[1]) for k in want if k[1] != "NaN"}
    assert sum(b + 1 in keys for b in keys) > 500                                           # an ulp apart: apart
    s = SamText(sam_of(texts))
    try:
        got = s.tag_values("XF")
    finally:
        s.close()
    wrong = sorted(set(got.items()) ^ set(want.items()))
    assert not wrong[:12], len(wrong)
    assert got == want


def test_midpoint_texts_through_arrow():
    texts = C.midpoint_texts()[::15]
    assert len(texts) == 200
    recs = [(b"NM:i:1\tXF:f:" + t, False) for t in texts]
    want = wanted_values(texts)
    for bits in (64, 4):
        assert arrow_values(table(recs, (7, 64, 100)), "XF", bits) == want, bits


def test_attributes_column():
    texts = sample()
    assert 200 <= len(texts) <= 260 and C.MIDPOINT_17[0] in texts and C.underflow_tie() + b"1" in texts
    s = SamText(sam_of(texts))
    try:
        t = A.adam_table(s, 0, len(texts), A.header_info(s))
        got = t.column("attributes").to_pylist()
    finally:
        s.close()
    assert not differing(got, ["XF:f:" + text_of(t) for t in texts], texts)


def test_bam_encoder_and_print_tags_store_the_same_float():
    """the BAM encoder (C strtof over the tag text) and print_tags read one float out of one text"""
    texts = [t for t in sample() if C.strtof_reads_alike(t)]
    assert len(texts) >= 200 and C.MIDPOINT_17[0] in texts
    s = SamText(sam_of(texts))
    try:
        raw = s.bam_records().tobytes()
        values = s.tag_values("XF")
    finally:
        s.close()
    stored, p = [], 0
    while p < len(raw):
        bs, = struct.unpack_from("<i", raw, p)
        tags = B.parse_record(raw[p + 4:p + 4 + bs])["tags"]
        assert tags[:3] == b"XFf" and len(tags) == 7
        stored.append(struct.unpack("<I", tags[3:])[0])
        p += 4 + bs
    assert not differing(stored, [C.parse_bits()[t] for t in texts], texts)
    assert values == dict(collections.Counter(("f", F.shortest_text(b)) for b in stored))
    assert sorted(bits_of_text(k[1]) for k in values) == sorted(set(stored))  # (no NaN among these texts)
