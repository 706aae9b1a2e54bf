"""MarkDuplicates' hand-built and random read sets (tests/_markdup_gen.py)
without a device: the expectation written beside each case, oracle/markdup.py
and the library's host form bqsr_mark_duplicates agree read by read; the
random sets exercise what they are meant to; the SAM rendering reads back as
the reads it was made from.  tests/test_gpu_markdup.py runs the same reads
through the device paths."""
import pytest

import markdup as M  # oracle/markdup.py
import _markdup_gen as G


@pytest.mark.parametrize("name", list(G.CASES))
def test_case_expectation_oracle_and_host_form(name):
    reads, want = G.case(name)
    assert M.mark_duplicates(reads) == want
    assert list(G.host_mark(reads)) == want


def test_cases_side_by_side_do_not_meet():
    reads, want = G.concat()
    assert M.mark_duplicates(reads) == want
    assert list(G.host_mark(reads)) == want
    sam_reads, sam_want = G.concat(sam_only=True)
    assert G.sam_ok(sam_reads) and 150 < len(sam_reads) < len(reads)
    assert M.mark_duplicates(sam_reads) == sam_want


def test_arrow_only_cases_are_the_expected_ones():
    only = {n for n in G.CASES if not G.sam_ok(G.case(n)[0])}
    assert only == {"reference_unmapped_reads", "names_that_are_prefixes_control_char", "empty_qual", "null_names",
                    "null_library", "libraries_within_one_bucket"}


@pytest.mark.parametrize("seed", G.RANDOM_SEEDS)
def test_random_set_exercises_every_feature(seed):
    reads = G.random_reads(2000, seed)
    assert len(reads) == 2000 and G.sam_ok(reads)
    got = G.coverage(reads)
    for key, floor in G.RANDOM_FLOOR.items():
        assert got[key] >= floor, (key, got)
    cigars = {"".join("%d%s" % e for e in r["cigar"]) for r in reads}
    assert set(G.RANDOM_CIGARS) <= cigars
    assert {r["ref"] for r in reads} == {None, 0, 1, 2} and {r["rg"] for r in reads} == {None, 0, 1, 2, 3}
    assert any(r["qual"] == "*" for r in reads) and any(ord(max(r["qual"])) >= 0xA1 for r in reads)


def test_small_random_set_is_not_trivial():
    got = G.coverage(G.random_reads(300, G.SMALL_SEED))  # the set the one-read partitions use
    assert all(v >= 1 for v in got.values()), got
    assert got["duplicate_primaries"] >= 20 and got["duplicate_secondaries"] >= 5


@pytest.mark.parametrize("seed", G.RANDOM_SEEDS)
def test_host_form_equals_oracle_on_random_sets(seed):
    reads = G.random_reads(2000, seed)
    assert list(G.host_mark(reads)) == M.mark_duplicates(reads)


def test_sam_rendering_reads_back_as_its_source():
    reads, _ = G.concat(sam_only=True)
    reads = reads + G.random_reads(300, G.SMALL_SEED)
    assert G.dicts_of_sam(G.sam_text(reads)) == reads


def test_bam_rendering_holds_the_reads_values():
    reads, _ = G.concat(sam_only=True)
    text = G.sam_text(reads)
    # the BAM writer is fed the SAM text: its records carry the same names, flags and positions
    import struct
    import zlib
    bam = G.bam_bytes(reads)
    raw, p = b"", 0
    while p < len(bam):
        bsize = struct.unpack_from("<H", bam, p + 16)[0] + 1
        raw += zlib.decompress(bam[p + 18:p + bsize - 8], -15)
        p += bsize
    l_text, = struct.unpack_from("<i", raw, 4)
    assert raw[8:8 + l_text] == G.header()
    q = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, q)
    q += 4
    for _ in range(n_ref):
        q += 8 + struct.unpack_from("<i", raw, q)[0]
    for r, f in zip(reads, G.sam_fields(text)):
        size, rid, pos, l_name, _mq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiiBBHHHi", raw, q)
        assert rid == (-1 if r["ref"] is None else r["ref"]) and pos == (-1 if r["start"] is None else r["start"])
        assert flag == int(f[1]) and n_cig == len(r["cigar"])
        assert raw[q + 36:q + 36 + l_name - 1].decode("latin-1") == r["name"]
        qual = raw[q + 36 + l_name + 4 * n_cig + (l_seq + 1) // 2:][:l_seq]
        if r["qual"] != "*":
            assert bytes((b + 33) & 0xFF for b in qual).decode("latin-1") == r["qual"]
        q += 4 + size
    assert q == len(raw)


def test_arrow_rendering_holds_the_reads_values():
    pa = pytest.importorskip("pyarrow")
    all_reads, _ = G.concat()
    t = G.arrow_table(all_reads)
    assert t.num_rows == len(all_reads)
    assert t.column("readName").to_pylist() == [r["name"] for r in all_reads]
    assert t.column("recordGroupLibrary").to_pylist() == [r["library"] for r in all_reads]
    assert t.column("referenceId").to_pylist() == [r["ref"] for r in all_reads]
    assert t.column("start").to_pylist() == [r["start"] for r in all_reads]
    assert t.column("qual").to_pylist() == [r["qual"] for r in all_reads]
    assert t.column("readName").null_count == sum(r["name"] is None for r in all_reads) >= 13
    assert t.column("start").null_count > 0 and t.column("referenceId").null_count > 0
    assert "" in t.column("readName").to_pylist() and "" in t.column("qual").to_pylist()
    assert t.schema.field("mateMapped").type == pa.bool_()
