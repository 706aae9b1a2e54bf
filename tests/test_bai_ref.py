"""tests/_bai_ref.py pinned without a device: one index spelled out by hand,
every generator shape accepted as sorted, the index-only reader against a scan
of all records, and the two refusals.  BAMs by adam_amd/bam_writer.sam_to_bam."""
import struct

import pytest

import _bai_gen as G
import _bai_ref as R
from adam_amd.bam_writer import sam_to_bam


@pytest.fixture(scope="module")
def bams():
    return {name: sam_to_bam(make()) for name, make in G.SHAPES.items()}


def test_three_reads_by_hand():
    """header: 4 + 4 + 19 + 4 + (4 + 2 + 4) = 41 bytes; a 30M record with a
    one-letter name is 4 + 32 + 2 + 4 + 15 + 30 = 87 bytes, without a CIGAR 83"""
    text = (b"@SQ\tSN:c\tLN:100000\n"
            + G.short(b"a", b"c", 101)                         # [100, 130): bin 4681, window 0
            + G.short(b"b", b"c", 20001)                       # [20000, 20030): bin 4682, window 1
            + G.short(b"c", b"c", 20001, flag=4, cigar=b"*")   # [20000, 20001): bin 4682, joins b's chunk
            + G.short(b"d", b"*", 0, flag=4, cigar=b"*"))      # unplaced
    bam = sam_to_bam(text)
    M = 0 << 16  # everything lies in the first member, at file offset 0
    assert struct.unpack_from("<I", bam, struct.unpack_from("<H", bam, 16)[0] + 1 - 4)[0] == 41 + 87 + 87 + 83 + 83
    want = (b"BAI\1" + struct.pack("<i", 1)
            + struct.pack("<i", 3)
            + struct.pack("<IiQQ", 4681, 1, M + 41, M + 128)
            + struct.pack("<IiQQ", 4682, 1, M + 128, M + 298)
            + struct.pack("<IiQQQQ", 37450, 2, M + 41, M + 298, 2, 1)
            + struct.pack("<iQQ", 2, M + 41, M + 128)
            + struct.pack("<Q", 1))
    assert R.bai_of_bam(bam) == want
    assert R.parse_bai(want) == dict(n_no_coor=1, refs=[dict(
        bins={4681: [(41, 128)], 4682: [(128, 298)], 37450: [(41, 298), (2, 1)]}, order=[4681, 4682, 37450],
        linear=[41, 128])])
    assert R.query(bam, want, 0, 20000, 20001) == [1, 2]
    assert R.query(bam, want, 0, 0, 100) == [] and R.query(bam, want, 0, 129, 130) == [0]


def test_a_record_that_ends_the_file_ends_in_the_eof_marker():
    bam = sam_to_bam(b"@SQ\tSN:c\tLN:100000\n" + G.short(b"a", b"c", 101))
    eof = len(bam) - 28
    assert R.parse_bai(R.bai_of_bam(bam))["refs"][0]["bins"][4681] == [(41, eof << 16)]


@pytest.mark.parametrize("name", sorted(G.SHAPES))
def test_shapes_are_sorted_and_readable(bams, name):
    bam = bams[name]
    bai = R.bai_of_bam(bam)  # no refusal: the GPU tests' inputs are in coordinate order
    P = R.parse_bai(bai)
    assert len(P["refs"]) == 3
    assert all(r["order"] == sorted(r["order"]) and (not r["order"] or r["order"][-1] == 37450) for r in P["refs"])
    for rid, beg, end in G.REGIONS:
        assert R.query(bam, bai, rid, beg, end) == R.scan(bam, rid, beg, end), (rid, beg, end)


def test_regions_find_something(bams):
    """the fixed regions are not all empty: each kind hits at least one shape where it should"""
    b = bams["bins_and_windows"]
    assert R.scan(b, 0, 0, 50000) == [] and R.scan(b, 0, 200000, 210000) == []
    for edge in (G.B14, G.B17, G.B26):
        assert len(R.scan(b, 0, edge - 10, edge + 10)) == 2  # the read across it and the one that starts on it
    assert len(R.scan(b, 0, 540000, 540001)) == 1  # inside the N of the five-window read
    assert R.scan(b, 1, 0, 1 << 29) == [] and len(R.scan(b, 2, 0, 1 << 29)) == 1
    lin = R.parse_bai(R.bai_of_bam(b))["refs"][0]["linear"]
    assert lin[:6] == [0] * 6 and lin[6] != 0           # the first read starts at 100 000
    assert lin[30] == lin[31] == lin[34] != lin[29]     # one read over five windows
    assert lin[40] == lin[34]                           # a gap takes the window before it


def test_chunk_runs_merge_and_split(bams):
    P = R.parse_bai(R.bai_of_bam(bams["chunk_runs"]))["refs"][0]["bins"]
    assert [len(P[4681 + w]) for w in (10, 20, 30)] == [1, 1, 1]
    leaf = P[4681 + ((G.B26 - 16000) >> 14)]
    assert 1 < len(leaf) < 10 and 1 < len(P[0]) < 10  # ten runs each: some merged, some split


def test_refusals_name_the_read():
    head = G.HEAD
    ok = [G.short(b"a", b"chr1", 100), G.short(b"b", b"chr1", 200), G.short(b"c", b"chr3", 50)]
    cases = {
        "start": (ok[:2] + [G.short(b"x", b"chr1", 150)], R.UNSORTED, 2),
        "refid": (ok + [G.short(b"x", b"chr1", 900)], R.UNSORTED, 3),
        "placed_after_unplaced": (ok + [G.short(b"u", b"*", 0, flag=4, cigar=b"*"), G.short(b"x", b"chr3", 60)],
                                  R.UNSORTED, 4),
        "limit": (ok[:2] + [G.short(b"x", b"chr1", (1 << 29) - 10)], R.UNSUPPORTED, 2),
        "both_on_one_read": (ok + [G.short(b"x", b"chr1", (1 << 29) - 10)], R.UNSORTED, 3),
    }
    for name, (recs, status, read) in cases.items():
        with pytest.raises(R.BaiRefusal) as e:
            R.bai_of_bam(sam_to_bam(head + b"".join(recs)))
        assert (e.value.status, e.value.read) == (status, read), name
    R.bai_of_bam(sam_to_bam(head + G.short(b"x", b"chr1", (1 << 29) - 29)))  # end == 2^29 is allowed
