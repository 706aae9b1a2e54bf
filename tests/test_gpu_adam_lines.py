"""adam2sam on the device: the SAM lines adam_amd/csrc/adam_lines.hip renders
from ADAMRecord columns (parquet.sam_text, python -m adam_amd.adam2sam)
against tests/_adam_lines_ref.py, the rules restated per record; then the
sinks over the result -- SAM text, BAM (tests/_bam_ref.py), its index
(tests/_bai_ref.py), the sort (tests/_sort_ref.py) -- and every refusal."""
import ctypes
import os

import numpy as np
import pytest

import _adam_lines_ref as R
import _bai_ref as BAI
import _bam_ref as B
import _sort_ref as S
from _adam_ref import convert_sam
from adam_amd import _capi, bqsr
from adam_amd import parquet as P
from adam_amd.adam2sam import adam2sam, main
from adam_amd.flagstat import arrow_flagstat, table_chunks
from adam_amd.sam import SamText
from adam_amd.transform import transform
from test_gpu_bam_out import file_stream

pytestmark = pytest.mark.gpu

RES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_resources")
FIXTURES = ["artificial.realigned.sam", "artificial.sam", "reads12.sam", "small.sam", "small_realignment_targets.sam",
            "unmapped.sam"]
SIZES = [0, 1, 63, 64, 65, 129]  # none, one lane, a wavefront less one, one, one and a lane, two and a lane
_CACHE = {}


def generated(n: int):
    """n records: the canonical generator's (its strings 0, 1, 63, 64, 65 and
    300 long, an attribute as long), one of them with every column null, some
    with single columns null or empty"""
    if n not in _CACHE:
        recs = convert_sam(R.canonical_sam(n, seed=7), R.run_date)
        for i, r in enumerate(recs):
            if i % 11 == 5:
                r["attributes"] = None
            if i % 13 == 6:
                r["readName"] = ""
            if i % 17 == 9:
                r["mismatchingPositions"] = ""
            if i % 19 == 4:
                r["mapq"] = None
        if n > 1:
            recs[min(n - 1, 40)] = {}
        _CACHE[n] = recs
    return _CACHE[n]


def device_text(recs, cuts=(), header=None) -> bytes:
    sam = P.sam_text(R.table(recs, cuts), header)
    try:
        assert sam.counts().n_reads == len(recs)
        assert set(sam.adam_lines) >= {"header_s", "chunks_s", "upload_ms", "len_ms", "write_ms", "parse_ms"}
        return sam.text()
    finally:
        sam.close()


def write_adam(path, recs, cuts=()):
    import pyarrow.parquet as pq
    pq.write_table(R.table(recs, cuts), str(path))
    return str(path)


# ---- the text against the restatement ----

@pytest.mark.parametrize("n", SIZES)
def test_generated_tables(n):
    recs = generated(n)
    assert device_text(recs) == R.header(recs) + R.lines(recs)


def test_three_record_batches_cut_off_the_byte():
    recs = generated(129)
    t = R.table(recs, cuts=(13, 77))
    assert [b.num_rows for b in t.to_batches()] == [13, 64, 52] and t.column("qual").chunk(1).offset % 8 == 5
    assert device_text(recs, cuts=(13, 77)) == R.header(recs) + R.lines(recs)


def test_one_live_lane_in_the_last_wavefront_of_every_batch():
    recs = generated(129)
    assert device_text(recs, cuts=(1, 66)) == R.header(recs) + R.lines(recs)  # batches of 1, 65 and 63


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures(name):
    with open(os.path.join(RES, name), "rb") as fh:
        text = fh.read()
    recs = convert_sam(text, R.run_date)
    assert device_text(recs) == R.header(recs) + R.lines(recs)
    assert device_text(recs, header=R.head(text)) == R.head(text) + R.lines(recs)


def test_flagstat_of_the_text_equals_flagstat_of_the_table():
    # (a read whose mate lies on another contig needs its mapq: flagstat refuses a null one, on either path)
    throws = lambda r: (r.get("mapq") is None and r.get("mateReference") is not None  # noqa: E731
                        and r.get("mateReference") != r.get("referenceName"))
    recs = [r for r in generated(129) if not throws(r)]
    assert 100 < len(recs) < 129
    t = R.table(recs, cuts=(50,))
    chunks, keep = table_chunks(t)
    want = arrow_flagstat(chunks)
    sam = P.sam_text(t)
    try:
        got = sam.flagstat()
    finally:
        sam.close()
    assert [m.counts() for m in got] == [m.counts() for m in want] and sum(want[1].counts()) > 0
    t = R.table(generated(129))
    chunks, keep = table_chunks(t)
    sam = P.sam_text(t)
    try:
        with pytest.raises(_capi.BQSRError) as a:
            arrow_flagstat(chunks)
        with pytest.raises(_capi.BQSRError) as b:
            sam.flagstat()
    finally:
        sam.close()
    assert (a.value.status, a.value.read) == (b.value.status, b.value.read) == (_capi.NULL_FIELD, 4)


# ---- the round trip ----

@pytest.fixture(scope="module")
def canon(tmp_path_factory):
    """(the canonical SAM text, its path, the .adam `transform` makes of it)"""
    d = tmp_path_factory.mktemp("canon")
    text = R.canonical_sam(300, seed=11)
    (d / "in.sam").write_bytes(text)
    transform(str(d / "in.sam"), str(d / "reads.adam"))
    return text, str(d / "in.sam"), str(d / "reads.adam")


def test_round_trip_with_the_header_of_the_source(canon, tmp_path):
    text, src, adam = canon
    out = str(tmp_path / "back.sam")
    st = adam2sam(adam, out, header_from=src)
    with open(out, "rb") as fh:
        assert fh.read() == text
    assert st["reads"] == 300 and {"read", "header", "lines", "emit", "close"} <= set(st["phases"])
    assert os.listdir(str(tmp_path)) == ["back.sam"]


def test_round_trip_with_the_synthesised_header(canon, tmp_path):
    text, _, adam = canon
    out = str(tmp_path / "back.sam")
    assert main([adam, out]) == 0
    with open(out, "rb") as fh:
        got = fh.read()
    assert R.body(got) == R.body(text)
    head = R.head(got)
    assert head == R.header(convert_sam(text, R.run_date)) and b"chrUn" not in head and b"@HD" not in head


def test_header_from_a_bam(canon, tmp_path):
    text, src, adam = canon
    transform(src, str(tmp_path / "src.bam"))
    adam2sam(adam, str(tmp_path / "back.sam"), header_from=str(tmp_path / "src.bam"))
    assert (tmp_path / "back.sam").read_bytes() == text


# ---- BAM output ----

def sortable(n: int, seed: int = 5) -> bytes:
    """canonical SAM without placed reads that -sort_reads puts last, which a coordinate-sorted BAM cannot end
    with: the unmapped ones, and those of FLAG 0 (no flag is read from a FLAG of 0: readMapped is false)"""
    text = R.canonical_sam(n, seed)
    last = lambda f: int(f[1]) & 4 or int(f[1]) == 0  # noqa: E731
    keep = [l for l in R.body(text).split(b"\n")[:-1] if not (last(l.split(b"\t")) and l.split(b"\t")[2] != b"*")]
    return R.head(text) + b"".join(l + b"\n" for l in keep)


def test_bam_is_the_encoding_of_the_rendered_text(tmp_path):
    recs = generated(129)
    text = R.header(recs) + R.lines(recs)
    adam = write_adam(tmp_path / "in.adam", recs, cuts=(30,))
    st = adam2sam(adam, str(tmp_path / "out.bam"), bam_piece_reads=50)
    got = file_stream((tmp_path / "out.bam").read_bytes())
    sam = SamText(text)
    try:
        assert got == sam.bam_header() + sam.bam_records().tobytes()
    finally:
        sam.close()
    assert got == B.stream(text)
    assert st["bam"]["record_bytes"] + len(B.header(text)[0]) == len(got) and st["reads"] == 129
    adam2sam(adam, str(tmp_path / "dev.bam"), bam_compressor="device")
    assert file_stream((tmp_path / "dev.bam").read_bytes()) == got
    assert sorted(os.listdir(str(tmp_path))) == ["dev.bam", "in.adam", "out.bam"]


def test_sort_reads_and_the_index(tmp_path):
    text = sortable(200)
    recs = convert_sam(text, R.run_date)
    rendered = R.head(text) + R.lines(recs)
    adam = write_adam(tmp_path / "in.adam", recs)
    (tmp_path / "h.sam").write_bytes(R.head(text))
    adam2sam(adam, str(tmp_path / "sorted.sam"), sort_reads=True, header_from=str(tmp_path / "h.sam"))
    want = S.sorted_sam(rendered)
    assert (tmp_path / "sorted.sam").read_bytes() == want and want != rendered
    for name, kw in (("host.bam", {}), ("dev.bam", dict(bam_compressor="device"))):
        out = str(tmp_path / name)
        st = adam2sam(adam, out, sort_reads=True, bam_index=True, header_from=str(tmp_path / "h.sam"), **kw)
        with open(out, "rb") as fh:
            bam = fh.read()
        assert file_stream(bam) == B.stream(want)
        with open(out + ".bai", "rb") as fh:
            assert fh.read() == BAI.bai_of_bam(bam)
        assert st["bam"]["index_bytes"] > 8 and "sort" in st["phases"]


def test_command_line_on_small_sam(tmp_path):
    """the .adam made from small.sam, written as an indexed BAM by the command.  The fixture's records are put in
    coordinate order first: half of them have FLAG 0, which -sort_reads (the reference's order) puts last"""
    with open(os.path.join(RES, "small.sam"), "rb") as fh:
        text = fh.read()
    text = R.head(text) + b"".join(sorted(R.body(text).splitlines(True), key=lambda l: int(l.split(b"\t")[3])))
    src = str(tmp_path / "small.sam")
    with open(src, "wb") as fh:
        fh.write(text)
    transform(src, str(tmp_path / "small.adam"))
    out = str(tmp_path / "small.bam")
    assert main([str(tmp_path / "small.adam"), out, "-bam_index", "-header_from", src]) == 0
    with open(out, "rb") as fh:
        bam = fh.read()
    with open(out + ".bai", "rb") as fh:
        assert fh.read() == BAI.bai_of_bam(bam)
    assert file_stream(bam) == B.stream(R.head(text) + R.lines(convert_sam(text, R.run_date)))
    assert len(BAI.walk(bam)[2]) == 20 and {l.split(b"\t")[1] for l in R.body(text).splitlines()} == {b"0", b"16"}


# ---- refusals ----

OK = dict(readName="r", sequence="ACGT", qual="IIII", cigar="4M", attributes="NM:i:1\tRG:Z:g", referenceId=0,
          referenceName="chr1", start=10, mapq=3, readMapped=True, primaryAlignment=True, mismatchingPositions="4")
UNSUPPORTED, MALFORMED = _capi.UNSUPPORTED, _capi.SAM_PARSE
REFUSALS = {"%s_%s" % (col, nm): ({col: "A%sB" % ch}, UNSUPPORTED)
            for col in ("readName", "cigar", "sequence", "qual", "mismatchingPositions")
            for nm, ch in (("tab", "\t"), ("lf", "\n"), ("cr", "\r"))}
REFUSALS.update({
    "attributes_lf": (dict(attributes="NM:i:1\tXZ:Z:a\nb"), UNSUPPORTED),
    "attributes_cr": (dict(attributes="XZ:Z:a\r"), UNSUPPORTED),
    "attribute_short": (dict(attributes="NM:i"), MALFORMED),
    "attribute_tag": (dict(attributes="NM:i:1\t1M:i:3"), MALFORMED),
    "attribute_tag2": (dict(attributes="N_:i:3"), MALFORMED),
    "attribute_type": (dict(attributes="NM:x:3\tRG:Z:g"), MALFORMED),
    "attribute_colon": (dict(attributes="NM:i;3"), MALFORMED),
    "attribute_empty_last": (dict(attributes="NM:i:1\t"), MALFORMED),
    "attribute_empty_first": (dict(attributes="\tNM:i:1"), MALFORMED),
    "attribute_empty_middle": (dict(attributes="NM:i:1\t\tXT:A:U"), MALFORMED),
    "start_negative": (dict(start=-1), UNSUPPORTED),
    "start_large": (dict(start=2 ** 31 - 1), UNSUPPORTED),
    "mate_start_negative": (dict(mateAlignmentStart=-5), UNSUPPORTED),
    "mate_start_large": (dict(mateAlignmentStart=2 ** 40), UNSUPPORTED),
    "mapq_negative": (dict(mapq=-1), UNSUPPORTED),
    "mapq_large": (dict(mapq=256), UNSUPPORTED),
})


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_name_the_record_and_leave_nothing(tmp_path, name):
    change, status = REFUSALS[name]
    with pytest.raises(R.Malformed if status == MALFORMED else R.Unrepresentable):
        R.line(dict(OK, **change))
    for at in (0, 64, 128):
        recs = [dict(OK, readName="r%d" % i) for i in range(129)]
        recs[at] = dict(OK, **change)
        if at == 0:  # a later record fails too: the first one is named
            recs[100] = dict(OK, start=-7)
        adam = write_adam(tmp_path / "in.adam", recs, cuts=(70,))
        for out in ("out.sam", "out.bam"):
            with pytest.raises(_capi.BQSRError) as e:
                adam2sam(adam, str(tmp_path / out), bam_index=out.endswith(".bam"))
            assert (e.value.status, e.value.read) == (status, at), str(e.value)
            assert "record %d" % at in str(e.value)
            assert os.listdir(str(tmp_path)) == ["in.adam"]


def test_the_limits_themselves_are_written():
    recs = [dict(OK, start=2 ** 31 - 2, mateAlignmentStart=0, mateReference="chr1", mateReferenceId=0, mapq=255),
            dict(OK, start=0, mapq=0, attributes="XB:B:c,1\tXH:H:1F\tX0:Z:")]
    text = device_text(recs)
    assert text == R.header(recs) + R.lines(recs)
    assert b"\t2147483647\t255\t4M\t=\t1\t0\t" in text and text.endswith(b"\tX0:Z:\tXH:H:1F\tXB:B:c,1\tMD:Z:4\n")


@pytest.mark.parametrize("column", ["reference", "mate_reference"])
@pytest.mark.parametrize("index", [1, -1])
def test_reference_index_outside_the_names(column, index):
    """(parquet.sam_text builds the indices itself: only the call can be handed one)"""
    L = P._lines_lib()
    ctx = bqsr.Context.get(0)
    for at in (0, 64, 128):
        ref = np.zeros(129, np.int32)
        ref[at] = index
        C = P._LinesChunk()
        C.n_reads = 129
        setattr(C, column, ref.ctypes.data)
        arr = (P._LinesChunk * 1)(C)
        blob, off = np.frombuffer(b"chr1", np.uint8), np.array([0, 4], np.int64)
        h = ctypes.c_void_p()
        head = b"@SQ\tSN:chr1\n"
        st = L.bqsr_arrow_sam_lines(ctx.handle, arr, 1, blob.ctypes.data, off.ctypes.data, 1, head, len(head), None,
                                    ctypes.byref(h))
        assert st == MALFORMED and L.bqsr_last_error_read() == at and not h
    ref[128] = 0  # all inside: every record's RNAME (or RNEXT) is the name
    st = L.bqsr_arrow_sam_lines(ctx.handle, arr, 1, blob.ctypes.data, off.ctypes.data, 1, head, len(head), None,
                                ctypes.byref(h))
    assert st == 0
    sam = SamText.adopt(h, ctx)
    try:
        line = b"*\t0\tchr1\t0\t255\t*\t*\t0\t0\t*\t*\n" if column == "reference" else b"*\t0\t*\t0\t0\t*\tchr1\t0\t0\t*\t*\n"
        assert sam.text() == head + line * 129
    finally:
        sam.close()


HEADER_CONFLICTS = {
    "two_names": ([dict(OK), dict(OK, referenceName="chr9")], "two names"),
    "two_ids": ([dict(OK), dict(OK, mateReference="chr1", mateReferenceId=3)], "two ids"),
    "two_lengths": ([dict(OK, referenceLength=5), dict(OK, referenceLength=6)], "two lengths"),
    "read_group": ([dict(OK, recordGroupName="g", recordGroupLibrary="a"),
                    dict(OK, recordGroupName="g", recordGroupLibrary="b")], "two values of recordGroupLibrary"),
}


@pytest.mark.parametrize("name", sorted(HEADER_CONFLICTS))
def test_header_conflicts_are_refused(tmp_path, name):
    recs, what = HEADER_CONFLICTS[name]
    with pytest.raises(ValueError):
        R.header(recs)
    adam = write_adam(tmp_path / "in.adam", recs)
    with pytest.raises(ValueError, match=what):
        adam2sam(adam, str(tmp_path / "out.bam"), bam_index=True)
    assert os.listdir(str(tmp_path)) == ["in.adam"]


@pytest.mark.parametrize("column", ["referenceName", "mateReference"])
def test_header_from_a_file_that_lacks_a_name(tmp_path, column):
    recs = [dict(OK, readName="r%d" % i) for i in range(70)]
    recs[66] = dict(OK, **{column: "chr2", column.replace("Name", "") + "Id": 1})
    adam = write_adam(tmp_path / "in.adam", recs, cuts=(64,))
    (tmp_path / "h.sam").write_bytes(b"@HD\tVN:1.4\n@SQ\tSN:chr1\tLN:100\n")
    with pytest.raises(ValueError, match="record 66: %s 'chr2' is not among" % column):
        adam2sam(adam, str(tmp_path / "out.sam"), header_from=str(tmp_path / "h.sam"))
    assert sorted(os.listdir(str(tmp_path))) == ["h.sam", "in.adam"]


# ---- qual chars above 0x7F ----

def test_non_ascii_qual(tmp_path):
    """a qual chunk with 2-byte UTF-8 chars: one byte c & 0xFF per Java char, QUAL as long as SEQ"""
    recs = [dict(OK, readName="r%d" % i) for i in range(66)]
    recs[65] = dict(OK, qual="I\u00e9\u0141I")  # U+00E9 -> 0xE9, U+0141 -> 0x41
    adam = write_adam(tmp_path / "in.adam", recs, cuts=(64,))  # (the second chunk alone is re-encoded)
    adam2sam(adam, str(tmp_path / "out.sam"))
    got = (tmp_path / "out.sam").read_bytes()
    want = [dict(r) for r in recs]
    want[65]["qual"] = "I\u00e9AI"
    assert got == R.header(recs) + R.lines(want)
    last = got.split(b"\n")[-2].split(b"\t")
    assert last[10] == b"I\xe9AI" and len(last[10]) == len(last[9])
    with pytest.raises(_capi.BQSRError) as e:
        adam2sam(adam, str(tmp_path / "out.bam"))
    assert (e.value.status, e.value.read) == (_capi.UNSUPPORTED, 65)
    assert sorted(os.listdir(str(tmp_path))) == ["in.adam", "out.sam"]
