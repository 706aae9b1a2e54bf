"""`adam mpileup` on the device (adam_amd/csrc/mpileup.hip, adam_amd/mpileup.py)
against the plain-Python restatement of PileupTraversable and MpileupCommand's
print loop (tests/_mpileup_ref.py): the text byte for byte, for SAM, BAM and
ADAM Parquet input, and every failure with the restatement's status and read."""
import ctypes
import functools
import os

import pytest

import _adam_ref
import _mpileup_gen as MG
import _mpileup_ref as MR
import _pileup_gen as G
from adam_amd import _capi, adam_save, bam_writer
from adam_amd import mpileup as M
from adam_amd import parquet as P
from adam_amd.sam import SamText

pytestmark = pytest.mark.gpu

RES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_resources")
MD_GOLDEN = ("artificial.sam", "artificial.realigned.sam", "small_realignment_targets.sam")


def sam_text_of(data, bam=False, window_bytes=None):
    s = SamText(data, bam=bam)
    try:
        return b"".join(s.mpileup(window_bytes))
    finally:
        s.close()


def records_table(recs):
    """ADAMRecord dicts as the Arrow table Parquet input decodes to"""
    import pyarrow as pa
    sch = adam_save.schema()
    return pa.table([pa.array([r.get(f.name) for r in recs], f.type) for f in sch], schema=sch)


def arrow_text_of(table):
    kept, rows = M._filtered(table)
    A = P.ArrowReads(kept, markdup=True)
    try:
        return b"".join(A.mpileup())
    except _capi.BQSRError as e:  # (the read's index in `table`, as the command reports it)
        raise M._input_row(e, rows) from None
    finally:
        A.close()


def want(recs) -> bytes:
    return MR.mpileup(recs).encode("latin-1")


# ---- golden inputs -------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def golden(name):
    with open(os.path.join(RES, name), "rb") as fh:
        data = fh.read()
    return data, want(_adam_ref.convert_sam(data, G.run_date))


@pytest.mark.parametrize("name", MD_GOLDEN)
def test_golden_sam_and_bam(name):
    data, text = golden(name)
    assert text
    assert sam_text_of(data) == text
    assert sam_text_of(bam_writer.sam_to_bam(data), bam=True) == text


@pytest.mark.parametrize("name", MD_GOLDEN)
def test_golden_adam_parquet(name, tmp_path):
    from adam_amd.transform import transform
    data, text = golden(name)
    adam = str(tmp_path / "in.adam")
    transform(os.path.join(RES, name), adam)
    out = str(tmp_path / "out.txt")
    st = M.mpileup(adam, out)
    with open(out, "rb") as fh:
        assert fh.read() == text
    assert st["lines"] == text.count(b"\n") and st["bytes"] == len(text)


# ---- generated reads -----------------------------------------------------------

FILTERED = [dict(flag=4), dict(flag=256), dict(flag=512 | 16), dict(flag=1024), dict(flag=0)]
CASES = {
    # event counts around a wavefront and a block, and across several blocks
    "events0": [(5, "*"), (6, "3S")],
    "events1": [(5, "1M")],
    "events63": [(5, "63M")],
    "events64": [(5, "64M")],
    "events65": [(5, "30M"), (20, "35M")],
    "events255": [(5, "100M"), (50, "155M")],
    "events256": [(5, "150M"), (50, "106M")],
    "events257": [(5, "150M"), (50, "107M")],
    "blocks": [(5 + 20 * i, "150M") for i in range(7)] + [(200, "40M5D40M"), (210, "50M3I50M")],
    # depth at one position: a line's events across wavefronts and blocks
    "depth1": [(7, "3M")],
    "depth64": [(7, "3M")] * 64,
    "depth65": [(7, "3M")] * 40 + [(7, "1M1D1M")] * 5 + [(7, "1M2I2M")] * 20,
    "depth300": [(7, "3M", dict(mismatch=0.3))] * 200 + [(7, "1M1D1M")] * 30 + [(7, "2M2I1M")] * 40 + [(8, "2M")] * 30,
    # digit boundaries of the position, the count and the inserted read's length
    "pos10": [(7, "5M")], "pos100": [(97, "5M")], "pos1000000": [(999997, "6M1I2M")],
    "counts": [(50, "1M")] * 9 + [(51, "1M")] * 10 + [(52, "1M")] * 99 + [(53, "1M")] * 100,
    "inslen": [(10, "1I"), (20, "4M1I4M"), (40, "4M2I4M"), (60, "49M1I49M"), (200, "50M1I49M"),
               (300, "500M1I499M")],
    # shapes
    "ins_last": [(10, "5M2I")], "ins_first": [(10, "2I5M")], "ins_twice": [(10, "3M2I1I3M")],
    "deletes": [(10, "3M4D3M"), (11, "2M1D2M2D2M")],
    "skips": [(10, "3M5N3M"), (12, "2S5M3S"), (14, "2H5M2H"), (16, "3M2P3M"), (18, "3M2=3M"), (20, "3M2X3M")],
    "no_events_between": [(10, "5M"), (11, "*"), (12, "5M", dict(md=None)), (13, "4M"), (13, "*", dict(md="3"))],
    "all_filtered": [(10 + i, "5M", FILTERED[i % 5]) for i in range(70)],
    "some_filtered": [(10 + i, "5M", FILTERED[i % 5] if i % 3 else {}) for i in range(70)],
    "segments": [(10, "5M2I", dict(rname="c1")), (12, "5M", dict(rname="c1")), (3, "4M1D2M", dict(rname="c2")),
                 (1, "6M", dict(rname="c1")), (11, "2I3M", dict(rname="c1"))],
    "mixed": [(100 + 3 * i, ("20M", "5M1I14M", "8M2D10M", "3S10M2N5M", "*", "6M1I1I3M2D4M")[i % 6],
               {} if i % 11 else FILTERED[i % 5]) for i in range(200)],
}


@functools.lru_cache(maxsize=None)
def case(name):
    text = MG.sam_text(CASES[name], seed=len(name))
    recs = MG.records(text)
    return text, recs, want(recs)


@pytest.mark.parametrize("name", sorted(CASES))
def test_generated(name):
    text, recs, exp = case(name)
    n_ev = sum(int(l.split(b" ")[3]) for l in exp.splitlines())
    if name.startswith("events"):
        assert n_ev == int(name[6:])
    if name.startswith("depth"):
        assert max(int(l.split(b" ")[3]) for l in exp.splitlines()) >= int(name[5:])
    if name == "all_filtered":
        assert exp == b""
    if name in ("ins_last", "inslen"):
        assert b" ? 1 +" in exp
    s = SamText(text)
    try:
        sz = M.sam_prepare(s)
        assert (sz.n_events, sz.n_lines, sz.text_bytes) == (n_ev, exp.count(b"\n"), len(exp))
        assert sz.n_reads == sum(1 for r in recs if MR.PR.locus_predicate(r))
        assert b"".join(M.sam_mpileup(s, sizes=sz)) == exp
    finally:
        s.close()


@pytest.mark.parametrize("name", ["blocks", "depth300", "inslen", "segments", "mixed", "all_filtered", "events0"])
def test_generated_bam_and_adam(name):
    text, recs, exp = case(name)
    assert sam_text_of(bam_writer.sam_to_bam(text), bam=True) == exp
    assert arrow_text_of(records_table(recs)) == exp


def test_no_reads():
    assert sam_text_of(G.HEADER) == b""
    assert arrow_text_of(records_table([])) == b""


def test_grid_does_not_matter():
    from adam_amd import bqsr
    text, recs, exp = case("mixed")
    for grid in (1, 3):  # every grid-stride loop through many passes
        with bqsr.Context.get(0).tuned(pileup_grid=grid):
            assert sam_text_of(text) == exp
            assert sam_text_of(text, window_bytes=300) == exp


# ---- windows -------------------------------------------------------------------

def text_call(s, line0, budget):
    buf = ctypes.create_string_buffer(max(1, budget))
    nl, nb = ctypes.c_int64(), ctypes.c_int64()
    _capi.check(M._lib().bqsr_sam_mpileup_text(s.ctx.handle, s.h, line0, budget, buf, None, ctypes.byref(nl),
                                               ctypes.byref(nb)))
    return nl.value, buf.raw[:nb.value]


def test_windows():
    text, recs, exp = case("mixed")
    lines = exp.splitlines(keepends=True)
    s = SamText(text)
    try:
        sz = M.sam_prepare(s)
        assert sz.n_lines == len(lines)
        k = 5
        upto = sum(len(l) for l in lines[:k])
        assert text_call(s, 0, upto) == (k, b"".join(lines[:k]))          # ends exactly at a line end
        assert text_call(s, 0, upto - 1) == (k - 1, b"".join(lines[:k - 1]))  # one byte short of it
        assert text_call(s, 0, len(exp)) == (len(lines), exp)
        assert text_call(s, 0, len(exp) + 1000) == (len(lines), exp)
        assert text_call(s, len(lines), 10) == (0, b"")
        got, i = [], 0
        while i < len(lines):  # one line per window
            n, t = text_call(s, i, len(lines[i]))
            assert n >= 1 and t == b"".join(lines[i:i + n])
            got.append(t)
            i += n
        assert b"".join(got) == exp
        long_line = max(range(len(lines)), key=lambda i: len(lines[i]))
        with pytest.raises(_capi.BQSRError) as e:
            text_call(s, long_line, len(lines[long_line]) - 1)
        assert e.value.status == _capi.INVALID_ARG and "takes %d bytes" % len(lines[long_line]) in str(e.value)
        for wb in (len(max(lines, key=len)), 100, 1000):
            assert b"".join(M.sam_mpileup(s, wb, sizes=sz)) == exp
    finally:
        s.close()


# ---- failures ------------------------------------------------------------------

OK = [(5, "4M", dict(flag=1024)), (6, "6M"), (8, "5M")]  # a filtered read first: input index != kept index
FAILS = {
    "lower_case_base": OK + [(9, "5M", dict(seq="ACgTA", md="5"))],
    "iupac_base": OK + [(9, "5M", dict(seq="ACRTA", md="5"))],
    "md_base_R": OK + [(9, "5M", dict(seq="ACGTA", md="2R2"))],
    "short_sequence": OK + [(9, "5M", dict(seq="ACG", md="5"))],
    "m_over_md_delete": OK + [(9, "5M", dict(seq="ACGTA", md="2^A2"))],
    "d_without_md_delete": OK + [(9, "2M1D2M", dict(seq="ACGT", md="5"))],
    "mapq_255": OK + [(9, "5M", dict(mapq=255))],
    "bad_md": OK + [(9, "5M", dict(md="A5"))],
    "unsorted_below_first": OK + [(2, "5M")],
    "unsorted_above_first": OK + [(7, "5M")],
    "conflict": OK + [(20, "1M", dict(seq="N", md="1")), (20, "1M", dict(seq="A", md="1"))],
}


def check_failure(run, recs):
    with pytest.raises(MR.MpileupThrow) as w:
        MR.mpileup(recs)
    with pytest.raises(_capi.BQSRError) as g:
        run()
    assert g.value.name == w.value.status
    if isinstance(w.value, MR.ReferenceConflict):
        assert g.value.read == w.value.position
        assert w.value.reference_name in str(g.value) and "position %d" % w.value.position in str(g.value)
    else:
        assert g.value.read == w.value.read and "read %d" % w.value.read in str(g.value)
    return w.value


@pytest.mark.parametrize("name", sorted(FAILS))
def test_failures(name):
    text = MG.sam_text(FAILS[name], seed=3)
    recs = MG.records(text)
    e = check_failure(lambda: sam_text_of(text), recs)
    if name.startswith("unsorted"):
        assert isinstance(e, MR.Unsorted) and e.read == 3
    elif name == "conflict":
        assert (e.reference_name, e.position) == ("c1", 20)
    else:
        assert e.read == 3 and e.status == {"mapq_255": "NULL_FIELD", "bad_md": "MD_PARSE"}.get(name, "PILEUP")


def test_null_reference_id_in_parquet(tmp_path):
    import pyarrow.parquet as pq
    recs = MG.records(MG.sam_text(OK + [(9, "5M"), (10, "5M")]))
    recs[3]["referenceId"] = None
    check_failure(lambda: arrow_text_of(records_table(recs)), recs)
    # the command names the read by its index in the file, the filtered ones counted
    path = str(tmp_path / "in.parquet")
    pq.write_table(records_table(recs), path)
    out = str(tmp_path / "out.txt")
    with pytest.raises(_capi.BQSRError) as g:
        M.mpileup(path, out)
    assert (g.value.name, g.value.read) == ("NULL_FIELD", 3) and "read 3" in str(g.value)
    assert os.listdir(str(tmp_path)) == ["in.parquet"]


# ---- the command ---------------------------------------------------------------

def test_cli_round_trip(tmp_path, capsys):
    text, recs, exp = case("mixed")
    inp = str(tmp_path / "in.sam")
    with open(inp, "wb") as fh:
        fh.write(text)
    out = str(tmp_path / "out.txt")
    assert M.main([inp, "-output", out, "-window_bytes", "4096"]) == 0
    with open(out, "rb") as fh:
        assert fh.read() == exp
    assert "lines=%d" % exp.count(b"\n") in capsys.readouterr().err
    bad = str(tmp_path / "bad.sam")
    with open(bad, "wb") as fh:
        fh.write(MG.sam_text(FAILS["unsorted_above_first"], seed=3))
    out2 = str(tmp_path / "out2.txt")
    with pytest.raises(_capi.BQSRError) as e:
        M.main([bad, "-output", out2])
    assert e.value.status == _capi.UNSORTED
    assert sorted(os.listdir(str(tmp_path))) == ["bad.sam", "in.sam", "out.txt"]


def test_stdout_only_after_the_checks(tmp_path):
    import io
    text, recs, exp = case("segments")
    inp = str(tmp_path / "in.sam")
    with open(inp, "wb") as fh:
        fh.write(text)
    sink = io.BytesIO()
    M.mpileup(inp, stdout=sink)
    assert sink.getvalue() == exp
    bad = str(tmp_path / "bad.sam")
    with open(bad, "wb") as fh:
        fh.write(MG.sam_text(FAILS["conflict"], seed=3))
    sink = io.BytesIO()
    with pytest.raises(_capi.BQSRError):
        M.mpileup(bad, stdout=sink)
    assert sink.getvalue() == b""
