"""`adam reads2ref` on the device (adam_amd/csrc/pileup.hip, adam_amd/
reads2ref.py) against the plain-Python restatement of
Reads2PileupProcessor.readToPileups (tests/_pileup_ref.py): every column and
every validity bit, exactly, for SAM, BAM and ADAM Parquet input."""
import functools
import glob
import os
import random

import pytest

import _adam_ref
import _pileup_gen as G
import _pileup_ref as PR
from adam_amd import _capi, adam_save, bam_writer, bqsr, reads2ref
from adam_amd import parquet as P
from adam_amd.sam import SamText

pytestmark = pytest.mark.gpu

RES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_resources")
MD_GOLDEN = ("artificial.sam", "artificial.realigned.sam", "small_realignment_targets.sam")
ROWS = "MIS"  # with these operators alone a generated read gives exactly read_len rows


def sam_table(data, r0=0, n=None, bam=False):
    s = SamText(data, bam=bam)
    try:
        return s.pileups(r0, n)
    finally:
        s.close()


def adam_records_table(recs):
    """ADAMRecord dicts as the Arrow table Parquet input decodes to"""
    import pyarrow as pa
    sch = adam_save.schema()
    return pa.table([pa.array([r.get(f.name) for r in recs], f.type) for f in sch], schema=sch)


def arrow_table(table, r0=0, n=None):
    A = P.ArrowReads(reads2ref.locus_filter(table))
    try:
        return A.pileups(r0, n)
    finally:
        A.close()


def kept(recs):
    return [r for r in recs if PR.locus_predicate(r)]


def read_output(path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    parts = sorted(glob.glob(os.path.join(path, "part-r-*.parquet")))
    assert parts and os.path.exists(os.path.join(path, "_SUCCESS"))
    return pa.concat_tables([pq.read_table(p) for p in parts])


# ---- golden inputs -------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def golden(name):
    data = open(os.path.join(RES, name), "rb").read()
    recs = _adam_ref.convert_sam(data, G.run_date)
    return data, recs


@pytest.mark.parametrize("name", MD_GOLDEN)
def test_golden_sam_and_bam(name):
    data, recs = golden(name)
    rows = PR.reads_to_pileups(recs)
    assert rows
    G.assert_rows(sam_table(data), rows)
    G.assert_rows(sam_table(bam_writer.sam_to_bam(data), bam=True), rows)


@pytest.mark.parametrize("name", MD_GOLDEN)
def test_golden_adam_parquet(name, tmp_path):
    from adam_amd.transform import transform
    data, recs = golden(name)
    out = str(tmp_path / "in.adam")
    transform(os.path.join(RES, name), out)
    rows = PR.reads_to_pileups(kept(recs))
    G.assert_rows(arrow_table(P.read_table(out, columns=reads2ref.PROJECTION)), rows)


# ---- generated reads -----------------------------------------------------------

E = (0, "nomd"), (5, "star"), (0, "skips")
SIZES = {
    "rows1": [(1, None, ROWS)], "rows63": [(63, None, ROWS)], "rows64": [(64, None, ROWS)],
    "rows65": [(65, None, ROWS)], "rows150": [(150, None, ROWS)],
    "rows255": [(100, None, ROWS), (155, None, ROWS)], "rows256": [(150, None, ROWS), (106, None, ROWS)],
    "rows257": [(150, None, ROWS), (107, None, ROWS)],
    "straddle": [(1, None), (63, None), (64, None), (65, None), (150, None), (40, None, ROWS), (50, None, ROWS)],
    "empty_runs": [E[0], E[1], E[2], (40, None), E[2], E[0], E[0], E[1], (70, None), (1, None), E[1], E[2], E[0]],
    "all_empty": [E[i % 3] for i in range(70)],
    "mixed": [(1 + (7 * i) % 90, None) if i % 5 else E[i % 3] for i in range(150)],
}


@pytest.mark.parametrize("case", sorted(SIZES))
def test_generated_sizes(case):
    text, recs, per = G.generated(tuple(SIZES[case]), 11)
    rows = G.flat(per)
    if case.startswith("rows"):
        assert len(rows) == int(case[4:])
    if case == "all_empty":
        assert not rows
    G.assert_rows(sam_table(text), rows)
    G.assert_rows(arrow_table(adam_records_table(recs)), PR.reads_to_pileups(kept(recs)))


def test_no_reads():
    assert sam_table(G.HEADER).num_rows == 0
    assert sam_table(G.HEADER).column_names == PR.FIELDS
    assert arrow_table(adam_records_table([])).num_rows == 0


def test_generated_bam():
    text, recs, per = G.generated(tuple((1 + (11 * i) % 120, None) for i in range(120)), 12, True)
    G.assert_rows(sam_table(bam_writer.sam_to_bam(text), bam=True), G.flat(per))


def test_range_calls():
    specs = tuple((20 + i % 31, None) if i % 7 else E[i % 3] for i in range(300))
    text, recs, per = G.generated(specs, 13)
    s = SamText(text)
    try:
        G.assert_rows(s.pileups(0, 300), G.flat(per))
        import pyarrow as pa
        pieces = [G.plain(s.pileups(a, n)) for a, n in ((0, 1), (1, 63), (64, 64), (128, 172))]
        assert pa.concat_tables(pieces).equals(G.plain(s.pileups()))
        G.assert_rows(s.pileups(64, 64), G.flat(per, 64, 128))
    finally:
        s.close()


LONG = 1024  # cycles of 1M 1I 1M 1D, then 1M: 4097 elements, 4097 rows


def long_line(i):
    return G.sam_line(i, random.Random(i),
                      ("1M1I1M1D" * LONG + "1M", "ACGT" * 768 + "A", b"I" * 3073, "2^A" * LONG + "1"),
                      flag=16, rname="c1", mapq=30)


@functools.lru_cache(maxsize=None)
def long_case():
    lines, recs, per = G.records(tuple((30 + i, None) for i in range(6)), 14)
    lines = lines[:3] + [long_line(100)] + lines[3:]
    text = G.HEADER + b"".join(lines)
    recs = _adam_ref.convert_sam(text, G.run_date)
    return text, recs, [PR.read_to_pileups(r) for r in recs]


def test_one_long_read():
    text, recs, per = long_case()
    assert len(per[3]) == 4 * LONG + 1
    alone = G.HEADER + long_line(100)
    G.assert_rows(sam_table(alone), per[3])
    G.assert_rows(sam_table(text), G.flat(per))
    G.assert_rows(arrow_table(adam_records_table(recs)), PR.reads_to_pileups(kept(recs)))


@functools.lru_cache(maxsize=None)
def stride_case():
    return G.generated(tuple((30 + i % 11, None) for i in range(20000)), 15)


def test_grid_stride():
    text, recs, per = stride_case()
    ctx = bqsr.Context.get(0)
    s = SamText(text)
    try:
        auto = G.plain(s.pileups())
        G.assert_rows(auto, G.flat(per))
        for g in (1, 2, 3):
            with ctx.tuned(pileup_grid=g):
                assert G.plain(s.pileups()).equals(auto), g
    finally:
        s.close()


# ---- errors ----------------------------------------------------------------------

def line(i, cigar, md, seq, qual=None, flag=16, rname="c1", pos=101):
    tags = [] if md is None else [b"MD:Z:" + md.encode()]
    qual = (b"I" * len(seq)) if qual is None else qual
    return b"\t".join([b"e%d" % i, b"%d" % flag, rname.encode(), b"%d" % pos, b"30", cigar.encode(), b"*", b"0", b"0",
                       seq.encode(), qual] + tags) + b"\n"


# the throwing kinds a SAM line can carry (null sequence / qual: the Parquet test)
BAD = {
    "null_start": (dict(cigar="*", md="", seq="A", rname="*"), "NULL_FIELD"),
    "null_start_pos0": (dict(cigar="1M", md="1", seq="A", pos=0), "NULL_FIELD"),
    "md_no_leading_digit": (dict(cigar="1M", md="A1", seq="A"), "MD_PARSE"),
    "md_caret_without_bases": (dict(cigar="1M", md="1^1", seq="A"), "MD_PARSE"),
    "md_no_trailing_digit": (dict(cigar="*", md="1A", seq="A"), "MD_PARSE"),
    "md_beyond_int": (dict(cigar="1M", md="2147483648", seq="A"), "MD_PARSE"),
    "seq_star": (dict(cigar="1M", md="1", seq="*", qual=b"*"), "PILEUP"),
    "seq_equals": (dict(cigar="2M", md="2", seq="A="), "PILEUP"),
    "seq_dot_clipped": (dict(cigar="1S1M", md="1", seq=".A"), "PILEUP"),
    "seq_lower": (dict(cigar="2M", md="2", seq="Ac"), "PILEUP"),
    "seq_lower_insert": (dict(cigar="1M1I1M", md="2", seq="AcG"), "PILEUP"),
    "seq_short_m": (dict(cigar="3M", md="3", seq="AC", qual=b"III"), "PILEUP"),
    "seq_short_i": (dict(cigar="1M2I", md="1", seq="AC", qual=b"III"), "PILEUP"),
    "seq_short_zero_i": (dict(cigar="1M3=0I", md="4", seq="AC", qual=b"III"), "PILEUP"),
    "seq_short_s": (dict(cigar="3S", md="", seq="AC", qual=b"III"), "PILEUP"),
    "qual_short": (dict(cigar="3M", md="3", seq="ACG", qual=b"II"), "PILEUP"),
    "m_on_delete": (dict(cigar="2M", md="1^A0", seq="AC"), "PILEUP"),
    "m_beyond_md": (dict(cigar="3M", md="2", seq="ACG"), "PILEUP"),
    "m_after_skip": (dict(cigar="1M3N1M", md="2", seq="AC"), "PILEUP"),
    "d_on_match": (dict(cigar="1M1D1M", md="3", seq="AC"), "PILEUP"),
    "d_on_mismatch": (dict(cigar="1M1D1M", md="1A1", seq="AC"), "PILEUP"),
    "trailing_d": (dict(cigar="2M1D", md="2^A0", seq="AC"), "PILEUP"),
    "unmapped": (dict(cigar="1M", md="1", seq="A", flag=4), "PILEUP"),
    "flag_zero": (dict(cigar="1M", md="1", seq="A", flag=0), "PILEUP"),
    "md_before_walk": (dict(cigar="1M", md="x", seq="*", qual=b"*", flag=4), "MD_PARSE"),
}


@functools.lru_cache(maxsize=None)
def good_lines(n):
    return G.records(tuple((20 + i % 23, None) for i in range(n)), 16)[0]


def failing(text, **tune):
    """(status name, read) of the call; no rows come back"""
    ctx = bqsr.Context.get(0)
    s = SamText(text)
    try:
        with ctx.tuned(**tune), pytest.raises(_capi.BQSRError) as e:
            s.pileups()
        L = _capi.lib()
        assert L.bqsr_last_error_read() == e.value.read
        return e.value.name, e.value.read
    finally:
        s.close()


@pytest.mark.parametrize("kind", sorted(BAD))
def test_each_throwing_kind(kind):
    spec, status = BAD[kind]
    bad = line(0, **spec)
    rec = _adam_ref.convert_sam(G.HEADER + bad)[0]
    with pytest.raises(PR.PileupThrow) as e:
        PR.read_to_pileups(rec)
    assert e.value.status == status  # the restatement agrees with the table above
    lines = list(good_lines(40))
    lines.insert(17, bad)
    assert failing(G.HEADER + b"".join(lines)) == (status, 17)
    assert failing(G.HEADER + bad) == (status, 0)


@pytest.mark.parametrize("first,second", [("md_no_leading_digit", "seq_lower"), ("seq_lower", "md_no_leading_digit"),
                                          ("null_start", "trailing_d"), ("unmapped", "null_start")])
def test_lowest_bad_read_wins(first, second):
    lines = list(good_lines(3000))
    lines[90] = line(90, **BAD[first][0])
    lines[2900] = line(2900, **BAD[second][0])  # beyond the first workgroups' reads
    assert failing(G.HEADER + b"".join(lines)) == (BAD[first][1], 90)


def test_bad_read_in_a_late_grid_stride_pass():
    lines = list(good_lines(3000))
    lines[2777] = line(2777, **BAD["d_on_match"][0])
    for g in (1, 2):
        assert failing(G.HEADER + b"".join(lines), pileup_grid=g) == ("PILEUP", 2777)


# ---- Parquet front end -----------------------------------------------------------

def base_rec(i, **kw):
    r = dict(readName="p%d" % i, sequence="ACGTA", qual="IJKLM", cigar="1S3M1I", mismatchingPositions="1c1",
             start=1000 + i, mapq=i % 60, referenceName="c1", referenceId=0, readMapped=True, primaryAlignment=True,
             failedVendorQualityChecks=False, duplicateRead=False, readNegativeStrand=bool(i & 1),
             recordGroupSample="s%d" % (i % 3), recordGroupLibrary=None if i % 4 == 0 else "lib",
             recordGroupRunDateEpoch=None if i % 5 else 1383820200000, recordGroupPredictedMedianInsertSize=i % 2)
    r.update(kw)
    return r


def test_parquet_locus_predicate_and_nulls():
    recs = []
    names = ("readMapped", "primaryAlignment", "failedVendorQualityChecks", "duplicateRead")
    for m in range(16):
        recs.append(base_rec(len(recs), **{k: bool(m >> j & 1) for j, k in enumerate(names)}))
    for k in names:
        recs.append(base_rec(len(recs), **{k: None}))
    recs.append(base_rec(len(recs), cigar=None))
    recs.append(base_rec(len(recs), mismatchingPositions=None))
    recs.append(base_rec(len(recs), mapq=None))
    recs.append(base_rec(len(recs), readName=None, referenceName=None, referenceId=None))
    recs.append(base_rec(len(recs), qual="~¡ÿIJ"))
    keep = kept(recs)
    assert len(keep) == 1 + 5 and sum(r["mismatchingPositions"] is None or r["cigar"] is None for r in keep) == 2
    rows = PR.reads_to_pileups(keep)
    assert any(r["mapQuality"] is None for r in rows) and any(r["readName"] is None for r in rows)
    G.assert_rows(arrow_table(adam_records_table(recs)), rows)


def test_parquet_chunks_not_multiples_of_64():
    import pyarrow as pa
    text, recs, per = G.generated(tuple((10 + i % 50, None) if i % 9 else E[i % 3] for i in range(400)), 17)
    t = adam_records_table(recs)
    cuts = (0, 1, 66, 193, 200, 399, 400)
    chunked = pa.concat_tables([t.slice(a, b - a) for a, b in zip(cuts, cuts[1:])])
    assert chunked.column("start").num_chunks == 6
    rows = PR.reads_to_pileups(kept(recs))
    G.assert_rows(arrow_table(chunked), rows)
    A = P.ArrowReads(reads2ref.locus_filter(chunked))
    try:  # ranges over the filtered reads, the mapq column handed over once
        n = A.n_reads
        pieces = [G.plain(A.pileups(a, b - a)) for a, b in ((0, 65), (65, n))]
        assert pa.concat_tables(pieces).equals(G.expected_table(rows))
    finally:
        A.close()


def test_duplicates_filtered_for_parquet_only():
    lines = [line(i, "3M", "3", "ACG", flag=16 | (1024 if i % 2 else 0)) for i in range(10)]
    text = G.HEADER + b"".join(lines)
    recs = _adam_ref.convert_sam(text)
    assert sum(r["duplicateRead"] for r in recs) == 5
    G.assert_rows(sam_table(text), PR.reads_to_pileups(recs))
    got = arrow_table(adam_records_table(recs))
    assert got.num_rows == 15
    G.assert_rows(got, PR.reads_to_pileups(kept(recs)))


def test_parquet_null_fields_status():
    for kw, status in ((dict(sequence=None), "NULL_FIELD"), (dict(qual=None), "NULL_FIELD"),
                       (dict(start=None), "NULL_FIELD"), (dict(sequence=None, mismatchingPositions=""), "NULL_FIELD"),
                       (dict(sequence=None, cigar="1M", mismatchingPositions=""), "PILEUP"),
                       (dict(qual=None, cigar="1D", mismatchingPositions="1"), "PILEUP")):
        recs = [base_rec(0), base_rec(1), base_rec(2, **kw), base_rec(3, sequence="acgta")]
        with pytest.raises(PR.PileupThrow) as e:
            PR.reads_to_pileups(recs)
        assert (e.value.status, e.value.read) == (status, 2)
        with pytest.raises(_capi.BQSRError) as g:
            arrow_table(adam_records_table(recs))
        assert (g.value.name, g.value.read) == (status, 2), kw


# ---- end to end ------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def e2e_case():
    return G.generated(tuple((25 + i % 40, None) if i % 6 else E[i % 3] for i in range(600)), 18, True)


def test_reads2ref_sam_partitions(tmp_path):
    text, recs, per = e2e_case()
    inp, out = str(tmp_path / "in.sam"), str(tmp_path / "out.adam")
    open(inp, "wb").write(text)
    st = reads2ref.reads2ref(inp, out, partition_bytes=len(text) // 4, part_reads=70)
    assert st["partitions"] >= 3 and st["reads"] == 600 and st["parts"] > 3
    got = read_output(out)
    assert got.column_names == PR.FIELDS
    assert got.schema.equals(adam_save.pileup_schema())
    G.assert_rows(got, G.flat(per))
    # -mapq is parsed and never read
    for q in (0, 60):
        o = str(tmp_path / ("q%d.adam" % q))
        assert reads2ref.main([inp, o, "-mapq", str(q), "-part_reads", "70",
                               "-partition_bytes", str(len(text) // 4)]) == 0
        assert read_output(o).equals(got)


def test_reads2ref_bam_and_adam(tmp_path):
    from adam_amd.transform import transform
    text, recs, per = e2e_case()
    sam, bam, adam = (str(tmp_path / n) for n in ("in.sam", "in.bam", "in.adam"))
    open(sam, "wb").write(text)
    open(bam, "wb").write(bam_writer.sam_to_bam(text))
    transform(sam, adam, part_reads=256)
    out = str(tmp_path / "from_bam.adam")
    reads2ref.reads2ref(bam, out, part_reads=129)
    G.assert_rows(read_output(out), G.flat(per))
    out = str(tmp_path / "from_adam.adam")
    st = reads2ref.reads2ref(adam, out, part_reads=100, compression="snappy")
    assert st["reads"] == len(kept(recs))
    G.assert_rows(read_output(out), PR.reads_to_pileups(kept(recs)))


def test_reads2ref_refusals(tmp_path):
    text, recs, per = e2e_case()
    inp, out = str(tmp_path / "in.sam"), str(tmp_path / "out.adam")
    open(inp, "wb").write(text)
    with pytest.raises(ValueError):
        reads2ref.reads2ref(inp, out, aggregate=True)
    with pytest.raises(SystemExit):
        reads2ref.main([inp, out, "-aggregate"])
    assert os.listdir(str(tmp_path)) == ["in.sam"]  # refused before any file is created
    reads2ref.reads2ref(inp, out)
    with pytest.raises(FileExistsError):
        reads2ref.reads2ref(inp, out)
    reads2ref.reads2ref(inp, out, overwrite=True, part_reads=200)
    G.assert_rows(read_output(out), G.flat(per))
    # a throwing input leaves no output; the error names the read's ordinal in the whole input
    lines = text[len(G.HEADER):].splitlines(True)
    lines[555] = line(555, **BAD["seq_lower"][0])
    bad, gone = str(tmp_path / "bad.sam"), str(tmp_path / "gone.adam")
    open(bad, "wb").write(G.HEADER + b"".join(lines))
    with pytest.raises(_capi.BQSRError) as e:
        reads2ref.reads2ref(bad, gone, partition_bytes=len(text) // 4, part_reads=64)
    assert (e.value.name, e.value.read) == ("PILEUP", 555)
    assert not os.path.lexists(gone) and not os.path.lexists(gone + ".partial")
