"""The restatement of PileupAggregator (tests/_pileup_agg_ref.py) against the
reference's own suite and against the semantics written out in
include/adam_sam.h: the yardstick is checked before the device is."""
import pytest

import _pileup_agg_ref as AG
import _pileup_ref as PR

INT_MIN = -(1 << 31)


def row(pos=1, ref=0, base="A", mq=30, sq=30, count=1, soft=0, rev=0, name="r", start=0, end=1, **kw):
    r = dict.fromkeys(PR.FIELDS)
    r.update(referenceId=ref, position=pos, readBase=base, mapQuality=mq, sangerQuality=sq, countAtPosition=count,
             numSoftClipped=soft, numReverseStrand=rev, readName=name, readStart=start, readEnd=end)
    r.update(kw)
    return r


def suite_row(**kw):
    """a record as PileupAggregationSuite builds it: unset fields null"""
    r = dict.fromkeys(PR.FIELDS)
    r.update(kw)
    return r


# ---- PileupAggregationSuite.scala, ported ------------------------------------------

def test_suite_two_different_bases_do_not_change():
    p0 = suite_row(position=1, readBase="A", mapQuality=10, sangerQuality=30, countAtPosition=1, numSoftClipped=0,
                   numReverseStrand=0)
    p1 = suite_row(position=1, readBase="C", mapQuality=20, sangerQuality=40, countAtPosition=1, numSoftClipped=1,
                   numReverseStrand=1)
    out = AG.flatten([p0, p1])
    assert len(out) == 2
    assert [o for o in out if o["readBase"] == "C"][0] == p1
    assert [o for o in out if o["readBase"] == "A"][0] == p0


@pytest.mark.parametrize("first,second,count", [((9, 31), (11, 29, 1, 1), 2), ((8, 32), (11, 29, 2, 2), 3)])
def test_suite_single_base_type(first, second, count):
    p0 = suite_row(position=1, readBase="A", mapQuality=first[0], sangerQuality=first[1], countAtPosition=1,
                   numSoftClipped=0, numReverseStrand=0, readName="read0", readStart=0, readEnd=1)
    p1 = suite_row(position=1, readBase="A", mapQuality=second[0], sangerQuality=second[1],
                   countAtPosition=second[2], numSoftClipped=second[3], numReverseStrand=second[3],
                   readName="read1", readStart=1, readEnd=2)
    (o,) = AG.flatten([p0, p1])
    assert (o["position"], o["readBase"], o["sangerQuality"], o["mapQuality"], o["countAtPosition"]) == \
        (1, "A", 30, 10, count)
    assert (o["numSoftClipped"], o["numReverseStrand"]) == (second[3], second[3])
    assert (o["readName"], o["readStart"], o["readEnd"]) == ("read0,read1", 0, 2)


# ---- the fold ------------------------------------------------------------------------

def test_worked_examples_depend_on_the_order():
    rows = [row(mq=q, sq=q, name="q%d" % q) for q in (10, 20, 30)]
    (o,) = AG.aggregate(rows)
    assert (o["mapQuality"], o["sangerQuality"], o["countAtPosition"], o["readName"]) == (30, 30, 3, "q10,q20,q30")
    (o,) = AG.aggregate(rows[::-1])
    assert (o["mapQuality"], o["sangerQuality"], o["readName"]) == (36, 36, "q30,q20,q10")


def test_fourteen_rows_wrap():
    """quality 60, count 1, 14 rows: M_k = M_{k-1} * (k - 1) + 60 over the integers
    passes 2^31 (it is factorial in depth); the fold is that number mod 2^32, as a
    signed int, divided the way Java divides"""
    m = 60
    for k in range(2, 15):
        m = m * (k - 1) + 60  # big integers, no wrapping
    assert m > 1 << 32
    w = m % (1 << 32)
    w = w - (1 << 32) if w >= 1 << 31 else w
    q = abs(w) // 14
    want = q if w >= 0 else -q
    (o,) = AG.aggregate([row(mq=60, sq=60, name="n") for _ in range(14)])
    assert (o["mapQuality"], o["sangerQuality"], o["countAtPosition"]) == (want, want, 14)
    assert want != m // 14


def test_java_division():
    assert AG.java_div(-7, 2) == -3 and AG.java_div(7, -2) == -3 and AG.java_div(-7, -2) == 3
    assert AG.java_div(INT_MIN, -1) == INT_MIN
    (o,) = AG.aggregate([row(mq=INT_MIN, sq=-9, count=-1)])
    assert (o["mapQuality"], o["sangerQuality"], o["countAtPosition"]) == (INT_MIN, 9, -1)


def test_single_row_is_divided_by_its_count():
    (o,) = AG.aggregate([row(mq=31, sq=20, count=3, soft=None, start=None)])
    assert (o["mapQuality"], o["sangerQuality"], o["countAtPosition"]) == (10, 6, 3)
    assert o["numSoftClipped"] is None and o["readStart"] is None  # a lone row passes through
    (again,) = AG.aggregate([o])
    assert (again["mapQuality"], again["sangerQuality"]) == (3, 2)  # aggregating twice divides twice


def test_sums_min_max_and_first_row_fields():
    rows = [row(soft=2, rev=1, start=5, end=9, referenceName="x", rangeLength=4, referenceBase="G"),
            row(soft=(1 << 31) - 1, rev=0, start=-3, end=7, referenceName="y", rangeLength=5, referenceBase="T")]
    (o,) = AG.aggregate(rows)
    assert (o["numSoftClipped"], o["numReverseStrand"], o["readStart"], o["readEnd"]) == (INT_MIN + 1, 1, -3, 9)
    assert (o["referenceName"], o["rangeLength"], o["referenceBase"]) == ("x", 4, "G")


# ---- grouping and the declared output order ------------------------------------------

def test_null_is_a_value_of_its_own_and_sorts_first():
    rows = [row(rangeOffset=0, name="zero"), row(name="null"), row(recordGroupSample="", name="empty"),
            row(base=None, name="nobase"), row(pos=-4, name="neg"), row(ref=-1, pos=9, name="negref"),
            row(recordGroupSample="b", name="b"), row(recordGroupSample="B", name="B"), row(rangeOffset=-2, name="m2"),
            row(base="D", name="D"), row(base="C", name="C")]
    out = AG.aggregate(rows)
    assert [o["readName"] for o in out] == ["negref", "neg", "nobase", "null", "empty", "B", "b", "m2", "zero", "C", "D"]
    assert all(o["countAtPosition"] == 1 for o in out)


# ---- strings -------------------------------------------------------------------------

def test_string_folds():
    def lib(*vals):
        (o,) = AG.aggregate([row(recordGroupLibrary=v) for v in vals])
        return o["recordGroupLibrary"]
    assert lib("X", "X", "Y", "X") == "X,Y,X"  # only a leading run collapses
    assert lib(None, "X") == "X" and lib("X", None) == "X" and lib(None, None) is None
    assert lib("X", "Y", "Y") == "X,Y,Y"
    assert lib("X", "X", "X") == "X"


def test_number_folds():
    def epoch(*vals):
        (o,) = AG.aggregate([row(recordGroupRunDateEpoch=v, recordGroupPredictedMedianInsertSize=v) for v in vals])
        assert o["recordGroupPredictedMedianInsertSize"] == o["recordGroupRunDateEpoch"]
        return o["recordGroupRunDateEpoch"]
    assert epoch(5, 7) is None
    assert epoch(5, 7, 7) == 7  # a later value sets it again
    assert epoch(5, None) == 5 and epoch(None, 5) == 5 and epoch(5, 5) == 5 and epoch(None, None) is None


def test_null_names():
    (o,) = AG.aggregate([row(name=None), row(name="b"), row(name=None)])
    assert o["readName"] == "null,b,null"
    (o,) = AG.aggregate([row(name=None)])
    assert o["readName"] is None
    a, b = row(name="x"), row(name=None)
    assert AG.reduce_step(a, b)["readName"] == "x,null"  # the step itself, as the Scala writes it


# ---- what throws ---------------------------------------------------------------------

def thrown(rows):
    with pytest.raises(AG.AggThrow) as e:
        AG.aggregate(rows)
    return e.value.status, e.value.row


@pytest.mark.parametrize("kw", [dict(ref=None), dict(pos=None), dict(mq=None), dict(sq=None), dict(count=None)])
def test_nulls_that_throw_in_every_row(kw):
    assert thrown([row(), row(pos=2, **{k: v for k, v in kw.items() if k != "pos"}) if "pos" not in kw
                   else row(pos=None), row(pos=3)]) == ("NULL_FIELD", 1)


@pytest.mark.parametrize("field", ["numSoftClipped", "numReverseStrand", "readStart", "readEnd"])
def test_nulls_that_throw_in_groups_of_two(field):
    assert AG.aggregate([row(pos=2), row(**{field: None})])[0][field] is None  # alone: passes through
    assert thrown([row(pos=2), row(), row(**{field: None}), row(**{field: None})]) == ("NULL_FIELD", 2)


def test_lowest_row_and_stages():
    rows = [row(pos=i % 5) for i in range(50)]
    rows[40]["mapQuality"] = None
    rows[30]["readEnd"] = None
    assert thrown(rows) == ("NULL_FIELD", 30)
    rows[45]["referenceId"] = None  # grouping throws before any fold does
    assert thrown(rows) == ("NULL_FIELD", 45)


def test_zero_count_is_pileup():
    assert thrown([row(pos=0), row(count=-5), row(pos=2), row(count=5)]) == ("PILEUP", 1)
    assert thrown([row(count=0)]) == ("PILEUP", 0)
    assert thrown([row(count=-5), row(count=5), row(count=None)]) == ("NULL_FIELD", 2)
    # the prediction of errors agrees with the fold itself
    with pytest.raises(ZeroDivisionError):
        AG.aggregate_pileup([row(count=-5), row(count=5)])
    with pytest.raises(AG.AggThrow):
        AG.aggregate_pileup([row(), row(rev=None)])
