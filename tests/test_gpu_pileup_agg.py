"""Pileup aggregation on the device (adam_amd/csrc/pileup_agg.hip, adam_amd/
aggregate_pileups.py) against the plain-Python restatement of PileupAggregator
(tests/_pileup_agg_ref.py) under the declared fold and output orders: every
column and every validity bit, exactly and in order."""
import functools
import os
import random

import numpy as np
import pytest

import _adam_ref
import _pileup_agg_ref as AG
import _pileup_gen as G
import _pileup_ref as PR
from adam_amd import _capi, aggregate_pileups as AP, bam_writer, bqsr, reads2ref

pytestmark = pytest.mark.gpu

INT_MIN = -(1 << 31)
WG = AP.WORKGROUP


def kept(recs):
    return [r for r in recs if PR.locus_predicate(r)]


def read_output(path):
    import glob

    import pyarrow as pa
    import pyarrow.parquet as pq
    parts = sorted(glob.glob(os.path.join(path, "part-r-*.parquet")))
    assert parts and os.path.exists(os.path.join(path, "_SUCCESS"))
    return pa.concat_tables([pq.read_table(p) for p in parts])


def aggregated(rows, adds=1):
    """the device's table of `rows` (restatement dicts), given in `adds` adds"""
    table = G.expected_table(rows)
    U = AP.Units()
    with AP.Aggregation() as agg:
        AP.add_pileup_table(agg, table, U, add_rows=max(1, -(-len(rows) // adds)))
        sz = agg.run()
        assert sz.n_rows == len(rows)
        F = agg.fetch(sz)
    U.freeze()
    return AP.group_table(F, U, 0, sz.n_groups)


def row(pos=1, ref=0, base="A", mq=30, sq=30, count=1, soft=0, rev=0, name="r", start=0, end=1, **kw):
    r = dict.fromkeys(PR.FIELDS)
    r.update(referenceId=ref, position=pos, readBase=base, mapQuality=mq, sangerQuality=sq, countAtPosition=count,
             numSoftClipped=soft, numReverseStrand=rev, readName=name, readStart=start, readEnd=end)
    r.update(kw)
    return r


def check(rows, adds=1):
    want = AG.aggregate(rows)
    G.assert_rows(aggregated(rows, adds), want)
    return want


# ---- PileupAggregationSuite (the suite calls flatten, which needs no referenceId:
# here the rows go through aggregate and carry referenceId 0) ----------------------

def test_suite_two_bases():
    rows = [row(base="A", mq=10, sq=30, name=None, start=None, end=None),
            row(base="C", mq=20, sq=40, soft=1, rev=1, name=None, start=None, end=None)]
    want = check(rows)
    assert [w["readBase"] for w in want] == ["A", "C"] and want == rows


@pytest.mark.parametrize("count,soft", [(1, 1), (2, 2)])
def test_suite_one_base(count, soft):
    rows = [row(mq=9 if count == 1 else 8, sq=31 if count == 1 else 32, name="read0", start=0, end=1),
            row(mq=11, sq=29, count=count, soft=soft, rev=soft, name="read1", start=1, end=2)]
    (w,) = check(rows)
    assert (w["sangerQuality"], w["mapQuality"], w["countAtPosition"], w["numSoftClipped"], w["readName"],
            w["readStart"], w["readEnd"]) == (30, 10, 1 + count, soft, "read0,read1", 0, 2)


# ---- random rows -----------------------------------------------------------------

RGS = [dict(recordGroupSample="s0", recordGroupLibrary="l0", recordGroupRunDateEpoch=5,
            recordGroupPredictedMedianInsertSize=300, recordGroupSequencingCenter="X"),
       dict(recordGroupSample="s0", recordGroupLibrary="l1", recordGroupRunDateEpoch=7,
            recordGroupSequencingCenter="X", recordGroupPlatform="p"),
       dict(recordGroupSample="s0", recordGroupLibrary="l0", recordGroupRunDateEpoch=5,
            recordGroupPredictedMedianInsertSize=250),
       dict(recordGroupSample="s1", recordGroupLibrary="l2", recordGroupDescription="d"),
       dict(recordGroupSample="", recordGroupFlowOrder="ACGT", recordGroupKeySequence="TG"),
       dict(recordGroupLibrary="l9", recordGroupPlatformUnit="u")]  # no sample


@functools.lru_cache(maxsize=None)
def random_case():
    rnd = random.Random(5)
    rows = []
    positions = list(range(-7, 13))  # 20 positions on each of 2 references: 40
    for i in range(5000):
        rg = rnd.choices(RGS, (8, 4, 2, 2, 1, 1))[0]
        ro = rnd.choices((None, 0, 1, -1), (12, 2, 1, 1))[0]
        rows.append(row(pos=rnd.choice(positions) if rnd.randrange(4) else 3, ref=rnd.choice((0, 1)),
                        base=rnd.choices((None, "A", "C", "D"), (1, 8, 2, 1))[0],
                        mq=rnd.randrange(0, 61), sq=rnd.randrange(-5, 94), count=rnd.choice((1, 1, 2, 3)),
                        soft=rnd.randrange(2), rev=rnd.randrange(2),
                        name=None if rnd.randrange(40) == 0 else "n%d" % i,
                        start=rnd.randrange(-100, 100), end=rnd.randrange(100, 300),
                        referenceName="c%d" % rnd.randrange(2) if rnd.randrange(9) else None,
                        rangeOffset=ro, rangeLength=None if ro is None else rnd.randrange(1, 9),
                        referenceBase=rnd.choice((None, "A", "G", "N")), **rg))
    want = AG.aggregate(rows)
    return rows, want


def test_random_rows():
    rows, want = random_case()
    sizes = {}
    for r in rows:
        k = (r["referenceId"], r["position"]) + AG.minor_key(r)
        sizes[k] = sizes.get(k, 0) + 1
    assert min(sizes.values()) == 1 and max(sizes.values()) > 200 and len(want) == len(sizes)
    assert any("," in (w["recordGroupLibrary"] or "") for w in want)  # the fold over several record groups
    G.assert_rows(aggregated(rows), want)


@pytest.mark.parametrize("grid", [1, 2, 3])
def test_grid_cap(grid):
    rows, want = random_case()
    with bqsr.Context.get(0).tuned(pileup_grid=grid):
        G.assert_rows(aggregated(rows), want)


@pytest.mark.parametrize("adds", [2, 3])
def test_split_adds(adds):
    rows, want = random_case()
    G.assert_rows(aggregated(rows, adds), want)


# ---- group sizes around the wavefront and the workgroup ---------------------------

SIZES = [1, 63, 64, 65, 62, WG - 1, WG, WG + 1, 2 * WG + 1, 1, 64, 3]


def test_size_boundaries():
    heads = np.cumsum([0] + SIZES[:-1])
    lanes = {int(h) % 64 for h in heads}
    assert 0 in lanes and 63 in lanes and len(lanes - {0, 63}) >= 2
    rnd = random.Random(6)
    rows = []
    for g, n in enumerate(SIZES):
        for k in range(n):
            rows.append(row(pos=10 + g, mq=rnd.randrange(61), sq=rnd.randrange(94), count=rnd.choice((1, 2, 3)),
                            soft=rnd.randrange(2), rev=rnd.randrange(2), name="g%d_%d" % (g, k),
                            start=rnd.randrange(1000), end=rnd.randrange(1000, 2000)))
    shuffled = rows[:]
    rnd.shuffle(shuffled)
    for case in (rows, shuffled):
        want = check(case)
        assert [w["countAtPosition"] for w in want] == [sum(r["countAtPosition"] for r in case if r["position"] == 10 + g)
                                                         for g in range(len(SIZES))]


def test_deep_group():
    rnd = random.Random(7)
    rows = [row(pos=4, mq=11, name="before")]
    rows += [row(pos=5, mq=rnd.randrange(61), sq=rnd.randrange(94), count=rnd.choice((1, 2, 3)), name="d",
                 rev=rnd.randrange(2)) for _ in range(70000)]
    rows += [row(pos=6, mq=13, name="after")]
    want = check(rows)
    assert [w["countAtPosition"] for w in want] == [1, sum(r["countAtPosition"] for r in rows[1:-1]), 1]


# ---- errors ------------------------------------------------------------------------

def fails(rows):
    with pytest.raises(AG.AggThrow) as want:
        AG.aggregate(rows)
    with pytest.raises(_capi.BQSRError) as got:
        aggregated(rows)
    assert (got.value.name, got.value.read) == (want.value.status, want.value.row)
    return got.value.name, got.value.read


@pytest.mark.parametrize("field", ["referenceId", "position", "mapQuality", "sangerQuality", "countAtPosition"])
def test_null_in_any_row(field):
    rows = [row(pos=i % 7) for i in range(600)]
    rows[577][field] = None
    rows[301][field] = None
    assert fails(rows) == ("NULL_FIELD", 301)
    assert fails([row(**{field: None}) if field not in ("referenceId", "position") else
                  row(**{"ref" if field == "referenceId" else "pos": None})]) == ("NULL_FIELD", 0)


@pytest.mark.parametrize("field", ["numSoftClipped", "numReverseStrand", "readStart", "readEnd"])
def test_null_in_a_group_of_two(field):
    lone = [row(pos=1), row(pos=2, **{field: None}), row(pos=3)]
    want = check(lone)
    assert want[1][field] is None
    rows = [row(pos=i % 7) for i in range(600)] + [row(pos=100, **{field: None})]
    rows[400][field] = None
    rows[333][field] = None
    assert fails(rows) == ("NULL_FIELD", 333)


def test_grouping_errors_come_first():
    rows = [row(pos=i % 7) for i in range(300)]
    rows[10]["mapQuality"] = None
    rows[200]["position"] = None
    assert fails(rows) == ("NULL_FIELD", 200)


def test_zero_count():
    rows = [row(pos=1), row(pos=2, count=-5, name="a"), row(pos=3), row(pos=2, count=5, name="b")]
    assert fails(rows) == ("PILEUP", 1)
    assert fails([row(count=0)]) == ("PILEUP", 0)
    # a null that throws in the same group throws first
    rows.append(row(pos=2, count=None))
    assert fails(rows) == ("NULL_FIELD", 4)


def test_int_min_by_minus_one():
    (w,) = check([row(mq=INT_MIN, sq=7, count=-1)])
    assert (w["mapQuality"], w["sangerQuality"], w["countAtPosition"]) == (INT_MIN, -7, -1)
    (w,) = check([row(mq=-7, sq=7, count=2)])
    assert (w["mapQuality"], w["sangerQuality"]) == (-3, 3)  # toward zero


def test_fetch_before_run():
    with AP.Aggregation() as agg:
        with pytest.raises(_capi.BQSRError) as e:
            agg.fetch(AP.AggSizes())
        assert e.value.name == "INVALID_ARG"
        sz = agg.run()
        assert (sz.n_rows, sz.n_groups) == (0, 0)


# ---- the command -------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def command_case():
    """_pileup_gen's end-to-end case with its reads moved onto a few hundred
    positions (so that groups form), mapq 255 (a null mapQuality, which
    aggregation throws on) replaced, and a fourth record group g3 that shares
    sample s0 with g0 under another library."""
    text, _, _ = G.generated(tuple((25 + i % 40, None) if i % 6 else ((0, "nomd"), (5, "star"), (0, "skips"))[i % 3]
                                   for i in range(600)), 18, True)
    header = G.HEADER + b"@RG\tID:g3\tSM:s0\tLB:lib3\tPL:other\n"
    lines = []
    for i, l in enumerate(text[len(G.HEADER):].splitlines(True)):
        f = l.split(b"\t")
        f[3] = b"%d" % (1000 + (i * 7) % 60)
        if f[4] == b"255":
            f[4] = b"13"
        l = b"\t".join(f)
        if i % 2:
            l = l.replace(b"RG:Z:g0", b"RG:Z:g3")
        lines.append(l)
    text = header + b"".join(lines)
    recs = _adam_ref.convert_sam(text, G.run_date)
    return text, recs


def test_command_all_inputs(tmp_path):
    from adam_amd.transform import transform
    text, recs = command_case()
    want = AG.aggregate(PR.reads_to_pileups(recs))
    assert any("," in (w["recordGroupLibrary"] or "") for w in want) and len(want) < len(PR.reads_to_pileups(recs))
    sam, bam, adam, pile = (str(tmp_path / n) for n in ("in.sam", "in.bam", "in.adam", "pile.adam"))
    open(sam, "wb").write(text)
    open(bam, "wb").write(bam_writer.sam_to_bam(text))
    transform(sam, adam, part_reads=256)
    reads2ref.reads2ref(sam, pile, part_reads=170)
    out = str(tmp_path / "from_sam.adam")
    st = AP.aggregate_pileups(sam, out, partition_bytes=len(text) // 3, part_reads=97, part_rows=500)
    assert st["reads"] == 600 and st["rows_out"] == len(want) and st["parts"] > 1
    got = read_output(out)
    from adam_amd import adam_save
    assert got.schema.equals(adam_save.pileup_schema())
    G.assert_rows(got, want)
    out = str(tmp_path / "from_bam.adam")
    AP.aggregate_pileups(bam, out, part_reads=131)
    G.assert_rows(read_output(out), want)
    out = str(tmp_path / "from_pileups.adam")
    assert AP.main([pile, out, "-parquet_compression", "snappy"]) == 0
    G.assert_rows(read_output(out), want)
    # ADAMRecord Parquet input: LocusPredicate applies
    out = str(tmp_path / "from_adam.adam")
    st = AP.aggregate_pileups(adam, out, part_reads=100)
    assert st["reads"] == len(kept(recs)) < len(recs)
    G.assert_rows(read_output(out), AG.aggregate(PR.reads_to_pileups(kept(recs))))


def test_command_throwing_input_leaves_nothing(tmp_path):
    text, recs = command_case()
    lines = text.splitlines(True)
    k = next(i for i, l in enumerate(lines) if not l.startswith(b"@") and b"MD:Z:" in l and l.split(b"\t")[5] != b"*")
    f = lines[k].split(b"\t")
    f[4] = b"255"  # no mapq: a null mapQuality in every row of the read
    lines[k] = b"\t".join(f)
    bad, out = str(tmp_path / "bad.sam"), str(tmp_path / "gone.adam")
    open(bad, "wb").write(b"".join(lines))
    with pytest.raises(_capi.BQSRError) as e:
        AP.aggregate_pileups(bad, out)
    assert e.value.name == "NULL_FIELD"
    assert os.listdir(str(tmp_path)) == ["bad.sam"]
    with pytest.raises(FileExistsError):
        open(out, "wb").close()
        AP.aggregate_pileups(bad, out)


def test_parquet_reads_without_reference_id(tmp_path):
    """ADAMRecord Parquet without its referenceId column: every row's referenceId is null, as in
    reads2ref's rows for it, and grouping throws on the first"""
    import pyarrow.parquet as pq
    from adam_amd.transform import transform
    text, recs = command_case()
    sam, adam, cut = (str(tmp_path / n) for n in ("in.sam", "in.adam", "cut.parquet"))
    open(sam, "wb").write(text)
    transform(sam, adam, part_reads=1000)
    pq.write_table(read_output(adam).drop(["referenceId"]), cut)
    with pytest.raises(_capi.BQSRError) as e:
        AP.aggregate_pileups(cut, str(tmp_path / "out.adam"))
    assert (e.value.name, e.value.read) == ("NULL_FIELD", 0)
    assert not os.path.exists(str(tmp_path / "out.adam"))
