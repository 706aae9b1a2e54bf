"""Indel realignment targets on the device (adam_amd/csrc/realign_targets.hip,
adam_amd/realignment_targets.py) against the plain-Python restatement of
RealignmentTargetFinder (tests/_realign_targets_ref.py): every result array
equal, for SAM, BAM and ADAM Parquet input, and every failure with the
restatement's status and read."""
import functools
import os

import numpy as np
import pytest

import _adam_ref
import _pileup_gen as G
import _pileup_ref as PR
import _realign_targets_gen as RG
import _realign_targets_ref as R
from adam_amd import _capi, adam_save, bam_writer
from adam_amd import parquet as P
from adam_amd import realignment_targets as RT
from adam_amd.sam import SamText

pytestmark = pytest.mark.gpu

RES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_resources")
GOLDEN = {"artificial.sam": (10, 650, 30, 1), "small_realignment_targets.sam": (7, 707, 17, 7),
          "artificial.realigned.sam": (10, 510, 20, 1)}
read = RG.read


def sam_run(data, bam=False):
    """(sizes, arrays) of a SAM / BAM text"""
    s = SamText(data, bam=bam)
    try:
        sz = RT.sam_prepare(s)
        return sz, RT.sam_targets(s, sizes=sz)
    finally:
        s.close()


def records_table(recs):
    """ADAMRecord dicts as the Arrow table Parquet input decodes to"""
    import pyarrow as pa
    sch = adam_save.schema()
    return pa.table([pa.array([r.get(f.name) for r in recs], f.type) for f in sch], schema=sch)


def arrow_run(recs):
    A = P.ArrowReads(records_table(recs))
    try:
        return A.realignment_targets()
    finally:
        A.close()


def assert_same(got, want):
    assert tuple(got) == RT.COLUMNS == R.COLUMNS
    for name in RT.COLUMNS:
        assert got[name].dtype == np.int64, name
        assert np.array_equal(got[name], want[name]), (name, got[name][:20], want[name][:20])


def check_sizes(sz, recs, targets, want):
    rows = PR.reads_to_pileups(recs)
    cands = [t for t in map(R.target_of_rod, R.group_rods(rows)) if not t.is_empty()]
    assert (sz.n_reads, sz.n_rows, sz.n_candidates, sz.n_targets, sz.n_indels, sz.n_snps) == \
        (len(recs), len(rows), len(cands), len(targets), len(want["indel_start"]), len(want["snp_site"]))


def check_text(text, recs=None):
    """SAM and BAM forms of `text` against the restatement; returns its targets"""
    recs = RG.records(text) if recs is None else recs
    targets = R.find_targets(recs)
    want = R.as_arrays(targets)
    sz, got = sam_run(text)
    check_sizes(sz, recs, targets, want)
    assert_same(got, want)
    sz, got = sam_run(bam_writer.sam_to_bam(text), bam=True)
    check_sizes(sz, recs, targets, want)
    assert_same(got, want)
    return targets


# ---- golden inputs -------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def golden(name):
    with open(os.path.join(RES, name), "rb") as fh:
        data = fh.read()
    return data, _adam_ref.convert_sam(data, G.run_date)


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_golden_sam_and_bam(name):
    data, recs = golden(name)
    targets = check_text(data, recs)
    sz, _ = sam_run(data)
    assert (sz.n_reads, sz.n_rows, sz.n_candidates, sz.n_targets) == GOLDEN[name]
    assert len(targets) == GOLDEN[name][3]


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_golden_adam_parquet(name, tmp_path):
    from adam_amd.transform import transform
    data, recs = golden(name)
    adam = str(tmp_path / "in.adam")
    transform(os.path.join(RES, name), adam)
    st = {}
    assert_same(RT.realignment_targets(adam, stats=st), R.as_arrays(R.find_targets(recs)))
    assert (st["reads"], st["rows"], st["candidates"], st["targets"]) == GOLDEN[name]


@pytest.mark.parametrize("name", ["reads12.sam", "small.sam", "unmapped.sam"])
def test_golden_without_md_gives_nothing(name):
    data, recs = golden(name)
    assert check_text(data, recs) == []


# ---- constructed cases ---------------------------------------------------------

def depth(d, zero, mis_qual="~"):
    """d reads 3M over one position, the middle one mismatching its middle
    base; `zero` of the matching reads carry quality 0, the others 1"""
    out = [read(500, "3M", "3", qual='"' * 3 if i >= zero else "!!!") for i in range(d - 1)]
    out.insert(d // 2, read(500, "3M", "1C1", qual=mis_qual * 3))
    return out


A20 = read(1, "4M1I16M", "20")   # candidate at 5 over [1, 20]
B = read(10, "2M1I4M", "6")      # candidate at 12 over [10, 15]
C14 = read(10, "4M1I17M", "21")  # candidate at 14 over [10, 30]
C11 = read(10, "1M1I20M", "21")  # candidate at 11 over [10, 30]

CASES = {
    # IndelRealignmentTargetSuite's make_read cases
    "suite_deletion": [read(3, "2M3D2M", "2^AAA2")],
    "suite_insertion": [read(3, "2M3I2M", "4")],
    "suite_same_deletion": [read(1, "4M3D2M", "4^AAA2"), read(2, "3M3D2M", "3^AAA2"), read(3, "2M3D2M", "2^AAA2")],
    "suite_two_indels": [read(1, "2M2D4M", "2^AA4"), read(1, "2M2D2M2D2M", "2^AA2^AA2"), read(5, "2M2D4M", "2^AA4")],
    "suite_disjoint": [read(1, "2M2D2M", "2^AA2"), read(7, "2M2D2M", "2^AA2")],
    # rod depth across a wavefront, a block and several tiles; the sums cross the carries
    "depth65_keep": depth(65, 0), "depth65_drop": depth(65, 0, mis_qual="*"),
    "depth257_keep": depth(257, 0), "depth257_drop": depth(257, 0, mis_qual="9"),
    "depth1025_keep": depth(1025, 600), "depth1025_drop": depth(1025, 0),
    # the threshold: 3 against 20 is exactly 0.15, 2 against 20 below; matchQuality 0 with matches; mismatches only
    "ratio_3_20": [read(40, "1M", "1", qual="5"), read(40, "1M", "0C0", qual="$")],
    "ratio_2_20": [read(40, "1M", "1", qual="5"), read(40, "1M", "0C0", qual="#")],
    "match_quality_0": [read(40, "1M", "1", qual="!"), read(40, "1M", "1", qual="!"), read(40, "1M", "0C0", qual="$")],
    "mismatches_only": [read(40, "1M", "0C0", qual="$"), read(40, "2M", "0C1", qual="!5")],
    "md_mismatch_naming_the_read_base": [read(40, "1M", "0A0", qual="5"), read(40, "1M", "0C0", qual="#")],
    # the fold
    "tie_inside_first": [C14, A20, B], "tie_beyond_first": [B, C11, A20],
    "partial_overlap": [A20, C14], "end_meets_start": [A20, read(20, "2M1I3M", "5")],
    "containment": [B, A20], "same_start": [read(1, "10M1I20M", "30"), A20],
    # the sets
    "single_rod_two_ranges": [read(100, "6M1I6M", "12"), read(102, "4M1I6M", "10")],
    "merged_one_range": [read(100, "6M2D6M", "6^AA6"), read(102, "4M2D6M", "4^AA6")],
    "insertion_of_3": [read(100, "6M3I6M", "12")],
    "soft_clips": [read(200, "2S3M", "3", qual="~~555"), read(200, "1M", "0C0", qual="#"), read(300, "4M3S", "4")],
    "no_rows_for_N_eq_X": [read(100, "3M2N3M", "8"), read(200, "2=2X3M", "7"), read(300, "3M2N1I3M", "8"),
                           read(400, "2=2X1I3M", "7"), read(500, "2H3M2P3M1I2M2H", "8")],
    "two_references_share_a_rod": [read(300, "1M", "1", qual="5", rname="c1"),
                                   read(300, "1M", "0C0", qual="#", rname="c2"),
                                   read(300, "1M", "0C0", qual="$", rname="c3"),
                                   read(700, "1M", "1", qual="5", rname="c1"), read(700, "1M", "0C0", qual="#", rname="c2")],
    "no_evidence": [read(10, "20M", "20"), read(15, "20M", "20"), read(5, "*", None), read(7, "5M", None)],
    "wide_quals": [read(40, "2M", "2", qual="\xfe\xa1"), read(40, "2M", "0C0C0", qual="\xff\x80")],
}
EXPECT_TARGETS = {"ratio_3_20": 1, "ratio_2_20": 0, "match_quality_0": 1, "mismatches_only": 1, "tie_inside_first": 2,
                  "md_mismatch_naming_the_read_base": 0,
                  "tie_beyond_first": 2, "partial_overlap": 2, "end_meets_start": 1, "containment": 1, "same_start": 1,
                  "single_rod_two_ranges": 1, "merged_one_range": 1, "insertion_of_3": 1, "no_evidence": 0,
                  "depth65_keep": 1, "depth65_drop": 0, "depth257_keep": 1, "depth257_drop": 0, "depth1025_keep": 1,
                  "depth1025_drop": 0, "two_references_share_a_rod": 1}


@pytest.mark.parametrize("name", sorted(CASES))
def test_constructed(name):
    text = RG.sam_text(CASES[name])
    if name == "wide_quals":  # (bytes beyond 0x7F are no BAM-safe quals: SAM only)
        recs = RG.records(text)
        targets = R.find_targets(recs)
        assert_same(sam_run(text)[1], R.as_arrays(targets))
    else:
        targets = check_text(text)
    if name in EXPECT_TARGETS:
        assert len(targets) == EXPECT_TARGETS[name]
    if name == "tie_inside_first":
        assert [len(t.indelSet) for t in targets] == [2, 1]
    if name == "tie_beyond_first":
        assert [len(t.indelSet) for t in targets] == [1, 2]
    if name == "single_rod_two_ranges":
        assert len(targets[0].indelSet) == 2 and targets[0].n_rods == 1
    if name == "merged_one_range":
        assert len(targets[0].indelSet) == 1 and targets[0].n_rods == 2 and targets[0].collapsed
        assert targets[0].indels()[0].readRange == R.Range(100, 113)
    if name == "insertion_of_3":
        assert len(targets[0].indelSet) == 1
    if name == "soft_clips":  # insert-type ranges at the clip position; the clip's quals count for nothing
        assert [(i.indelRange, i.readRange) for t in targets for i in t.indels()] == \
            [(R.Range(200, 200), R.Range(200, 202)), (R.Range(304, 304), R.Range(300, 303))]
        assert not any(t.snpSet for t in targets)
    if name == "no_rows_for_N_eq_X":
        assert [i.indelRange.start for t in targets for i in t.indels()] == [305, 404, 506]
    if name.startswith("depth"):
        assert max(len(r) for r in R.group_rods(PR.reads_to_pileups(RG.records(text)))) == int(name[5:].split("_")[0])


def test_no_reads():
    sz, got = sam_run(G.HEADER)
    assert (sz.n_reads, sz.n_rows, sz.n_targets) == (0, 0, 0)
    assert_same(got, R.as_arrays([]))
    assert_same(arrow_run([]), R.as_arrays([]))


# ---- a few thousand overlapping reads --------------------------------------------

@functools.lru_cache(maxsize=None)
def generated():
    text = RG.sam_text(RG.overlapping())
    recs = RG.records(text)
    targets = R.find_targets(recs)
    return text, recs, targets


def test_generated_reaches_every_kind_of_target():
    _, _, targets = generated()
    assert any(t.n_rods == 1 for t in targets)
    assert any(t.n_rods >= 2 for t in targets)
    assert any(t.snpSet for t in targets)
    assert any(t.collapsed for t in targets)
    assert any(t.n_rods == 1 and len({i.indelRange for i in t.indelSet}) < len(t.indelSet) for t in targets)
    assert len(targets) > 20


def test_generated_sam_and_bam():
    text, recs, targets = generated()
    assert check_text(text, recs) is not None


def test_generated_adam_parquet_and_arrow(tmp_path):
    from adam_amd.transform import transform
    text, recs, targets = generated()
    want = R.as_arrays(targets)
    assert_same(arrow_run(recs), want)
    inp = str(tmp_path / "in.sam")
    with open(inp, "wb") as fh:
        fh.write(text)
    adam = str(tmp_path / "in.adam")
    transform(inp, adam)
    assert_same(RT.realignment_targets(adam), want)


def test_grid_does_not_matter():
    from adam_amd import bqsr
    text, recs, targets = generated()
    want = R.as_arrays(targets)
    for grid in (1, 3):  # every grid-stride loop through many passes
        with bqsr.Context.get(0).tuned(pileup_grid=grid):
            assert_same(sam_run(text)[1], want)


# ---- failures ------------------------------------------------------------------

GOOD = [read(10, "5M1I5M", "10"), read(12, "6M", "2C3"), read(300, "4M2D4M", "4^AC4")]
THROWS = {
    "NULL_FIELD": read(-1, "5M", "5"),                    # POS 0: a null start
    "MD_PARSE": read(20, "5M", "A5"),
    "PILEUP": read(20, "5M", "5", seq="AAA", qual="AAA"),  # a sequence shorter than the CIGAR
}


def check_failure(run, recs):
    with pytest.raises(PR.PileupThrow) as w:
        R.find_targets(recs)
    with pytest.raises(_capi.BQSRError) as g:
        run()
    assert g.value.name == w.value.status
    assert g.value.read == w.value.read and "read %d" % w.value.read in str(g.value)
    assert RT._lib().bqsr_last_error_read() == w.value.read
    return w.value


@pytest.mark.parametrize("status", sorted(THROWS))
@pytest.mark.parametrize("where", [0, 2, 4])
def test_read_level_failures(status, where):
    reads = GOOD + [read(400 + 10 * k, "3M1I3M", "6") for k in range(2)]
    reads[where] = THROWS[status]
    if where == 0:  # a later read throws something else: the first one decides
        reads[3] = THROWS["MD_PARSE" if status != "MD_PARSE" else "PILEUP"]
    text = RG.sam_text(reads)
    recs = RG.records(text)
    e = check_failure(lambda: sam_run(text), recs)
    assert (e.status, e.read) == (status, where)
    check_failure(lambda: sam_run(bam_writer.sam_to_bam(text), bam=True), recs)
    check_failure(lambda: arrow_run(recs), recs)


def test_flag_0_with_cigar_and_md_is_pileup():
    text = RG.sam_text(GOOD + [read(50, "5M", "5", flag=0)])
    e = check_failure(lambda: sam_run(text), RG.records(text))
    assert (e.status, e.read) == ("PILEUP", 3)
    text = RG.sam_text([read(50, "5M", "5", flag=4)] + GOOD)  # an unmapped read
    e = check_failure(lambda: sam_run(text), RG.records(text))
    assert (e.status, e.read) == ("PILEUP", 0)


@pytest.mark.parametrize("where", [0, 2, 4])
def test_start_below_0_with_rows_is_unsupported(where):
    # (SAM cannot say it: POS 0 is a null start)
    recs = RG.records(RG.sam_text(GOOD + [read(50, "5M", "5"), read(60, "5M", "5")]))
    recs[where]["start"] = -1
    e = check_failure(lambda: arrow_run(recs), recs)
    assert (e.status, e.read) == ("UNSUPPORTED", where)
    recs[where]["cigar"] = None  # without rows it is no one's business
    assert_same(arrow_run(recs), R.as_arrays(R.find_targets(recs)))


# ---- the command ---------------------------------------------------------------

def test_cli(tmp_path, capsys):
    text, recs, targets = generated()
    inp = str(tmp_path / "in.sam")
    with open(inp, "wb") as fh:
        fh.write(text)
    out = str(tmp_path / "out.txt")
    assert RT.main([inp, "-output", out]) == 0
    with open(out) as fh:
        assert fh.read() == R.text(targets)
    assert "targets=%d" % len(targets) in capsys.readouterr().err
    only = str(tmp_path / "only.txt")
    assert RT.main([inp, "-output", only, "-targets_only"]) == 0
    with open(only) as fh:
        assert fh.read() == R.text(targets, targets_only=True)
    # a failure: no partial output and no file
    bad = str(tmp_path / "bad.sam")
    with open(bad, "wb") as fh:
        fh.write(RG.sam_text(GOOD + [THROWS["MD_PARSE"]]))
    with pytest.raises(_capi.BQSRError) as e:
        RT.main([bad, "-output", str(tmp_path / "bad.txt")])
    assert (e.value.name, e.value.read) == ("MD_PARSE", 3)
    assert sorted(os.listdir(str(tmp_path))) == ["bad.sam", "in.sam", "only.txt", "out.txt"]
    import io
    sink = io.BytesIO()
    with pytest.raises(_capi.BQSRError):
        RT.write_targets(bad, stdout=sink)
    assert sink.getvalue() == b""
    # no reads, and reads without evidence: an empty file
    for k, t in enumerate((G.HEADER, RG.sam_text(CASES["no_evidence"]))):
        p, o = str(tmp_path / ("none%d.sam" % k)), str(tmp_path / ("none%d.txt" % k))
        with open(p, "wb") as fh:
            fh.write(t)
        assert RT.main([p, "-output", o]) == 0
        assert os.path.getsize(o) == 0
