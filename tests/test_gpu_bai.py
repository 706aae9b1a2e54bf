"""`transform OUT.bam -bam_index`: the .bai the device builds while the BAM is
written (adam_amd/csrc/bam_index.hip, transform._BamOut) against
tests/_bai_ref.py, the index restated from the finished file alone.  Every
case asserts OUT.bam.bai == bai_of_bam(OUT.bam) byte for byte and reads regions
back through the index."""
import bisect
import os

import pytest

import _bai_gen as G
import _bai_ref as R
import _bam_ref as B
from adam_amd import _capi, synth
from adam_amd.bam_writer import sam_to_bam
from adam_amd.samgen import sam_text
from adam_amd.transform import BAM_INDEX_KERNELS, main, transform
from test_gpu_bam_out import file_stream

pytestmark = pytest.mark.gpu

WHOLE = (0, 0, 1 << 29)


def run(tmp_path, text: bytes, inp="in.sam", **kw):
    """(OUT.bam, OUT.bam.bai, stats) of transform -bam_index over `text`"""
    src = tmp_path / inp
    src.write_bytes(text)
    out = str(tmp_path / "out.bam")
    st = transform(str(src), out, bam_index=True, **kw)
    with open(out, "rb") as fh:
        bam = fh.read()
    with open(out + ".bai", "rb") as fh:
        bai = fh.read()
    assert not os.path.exists(out + ".partial") and not os.path.exists(out + ".bai.partial")
    assert st["bam"]["index_bytes"] == len(bai) and tuple(st["bam"]["index_ms"]) == BAM_INDEX_KERNELS
    return bam, bai, st


def check(bam: bytes, bai: bytes, regions):
    assert bai == R.bai_of_bam(bam)
    for rid, beg, end in regions:
        assert R.query(bam, bai, rid, beg, end) == R.scan(bam, rid, beg, end), (rid, beg, end)


SINKS = {"level0": dict(bam_level=0), "level6": dict(bam_level=6), "device": dict(bam_compressor="device")}


@pytest.mark.parametrize("sink", sorted(SINKS))
@pytest.mark.parametrize("shape", sorted(G.SHAPES))
def test_shapes_through_every_sink(tmp_path, shape, sink):
    bam, bai, _ = run(tmp_path, G.SHAPES[shape](), **SINKS[sink])
    check(bam, bai, G.REGIONS if sink == "level6" else [WHOLE, (0, G.B26 - 10, G.B26 + 10)])


@pytest.mark.parametrize("piece", [64, None])
def test_members_and_pieces(tmp_path, piece):
    """about ten records a member: records that straddle two members, pieces
    that end in short members, an index across many pieces"""
    kw = {} if piece is None else dict(bam_piece_reads=piece)
    bam, bai, _ = run(tmp_path, G.long_reads(), **kw)
    check(bam, bai, [WHOLE, (0, 105000, 105001)])
    S, _, recs = R.walk(bam)
    short = sum(1 for raw in S.raw[1:-1] if len(raw) < 65280)
    assert short == (5 if piece else 1) and len(S.raw) > 28
    member = lambda p: bisect.bisect_right(S.start, p) - 1  # noqa: E731  (of a stream position)
    assert sum(1 for r in recs if member(S.pos(r[4])) != member(S.pos(r[5]) - 1)) > 20  # records across two members
    if piece:  # the pieces' last records end on a member boundary: offset 0 in the member after it
        assert sum(1 for r in recs if r[5] & 0xFFFF == 0) >= 5


@pytest.mark.parametrize("tail", [70, 0])
def test_record_ends_exactly_on_a_member_boundary(tmp_path, tail):
    bam, bai, _ = run(tmp_path, G.exact_member(tail))
    check(bam, bai, [WHOLE, (0, 1500, 1501)])
    S, _, recs = R.walk(bam)
    assert len(S.raw[1]) == 65280 and recs[0][4] == S.file_off[1] << 16 and recs[0][5] == S.file_off[2] << 16
    assert len(S.raw) == (4 if tail else 3)  # header, the full member, (the tail,) the EOF marker
    if not tail:
        assert S.file_off[2] == len(bam) - 28


def test_chunks_merge_and_split(tmp_path):
    bam, bai, st = run(tmp_path, G.chunk_runs())
    check(bam, bai, [WHOLE, (0, G.B26 - 16000, G.B26 - 15990)])
    bins = R.parse_bai(bai)["refs"][0]["bins"]
    assert [len(bins[4681 + w]) for w in (10, 20, 30)] == [1, 1, 1]
    leaf = bins[4681 + ((G.B26 - 16000) >> 14)]
    assert 1 < len(leaf) < 10 and 1 < len(bins[0]) < 10  # ten runs each: merged ones and split ones
    assert st["bam"]["index_chunks"] == sum(len(c) for b, c in bins.items() if b != R.PSEUDO_BIN)


def test_references_and_header_only(tmp_path):
    bam, bai, _ = run(tmp_path, G.references())
    check(bam, bai, G.REGIONS)
    P = R.parse_bai(bai)
    assert P["n_no_coor"] == 3 and P["refs"][1] == dict(bins={}, order=[], linear=[])
    assert P["refs"][0]["bins"][R.PSEUDO_BIN][1] == (3, 1) and P["refs"][2]["bins"][R.PSEUDO_BIN][1] == (1, 1)
    assert 4681 in P["refs"][0]["bins"]  # POS 0: beg clamped to 0 (its bin field in the record stays 4680)
    os.remove(str(tmp_path / "out.bam")), os.remove(str(tmp_path / "out.bam.bai"))
    bam, bai, _ = run(tmp_path, G.header_only())
    check(bam, bai, [WHOLE])
    assert R.parse_bai(bai) == dict(n_no_coor=0, refs=[dict(bins={}, order=[], linear=[])] * 3)


# ---- through the pipeline ----

def test_partitions_and_bam_input(tmp_path):
    text = G.chunk_runs()
    bam, bai, st = run(tmp_path, text, mark_duplicates=True, partition_bytes=len(text) // 5)
    assert st["partitions"] >= 4
    check(bam, bai, [WHOLE, (0, G.B26 - 10, G.B26 + 10)])
    os.remove(str(tmp_path / "out.bam")), os.remove(str(tmp_path / "out.bam.bai"))
    bam2, bai2, _ = run(tmp_path, sam_to_bam(G.bins_and_windows()), inp="in.bam")
    check(bam2, bai2, G.REGIONS)


def test_markdup_and_recalibrate(tmp_path):
    # the generator seed tests/test_gpu_bam_out.py recalibrates into BAM, its records in coordinate order
    text = G.sort_text(sam_text(synth.generate(2000, lens=(100,), n_rg=2, seed=15, p_q2tail=0.0), n_rg=2))
    bam, bai, st = run(tmp_path, text, mark_duplicates=True, recalibrate=True)
    check(bam, bai, [WHOLE, (0, 0, 1 << 20)])
    assert st["reads"] == 2000 and len(R.walk(bam)[2]) == 2000


def unsorted_input(placed_unmapped: bool) -> bytes:
    recs = [G.short(b"m%d" % i, b"chr3" if i % 3 == 0 else b"chr1", 1 + (i * 7919) % 100000, flag=16)
            for i in range(300)]
    recs += [G.rec(b"u%d" % i, 4, b"*", 0, b"*", b"ACGTA") for i in range(3)]
    if placed_unmapped:
        recs.insert(10, G.short(b"pu", b"chr1", 5, flag=4, cigar=b"*"))
    return G.HEAD + b"".join(recs)


def test_sort_reads(tmp_path):
    bam, bai, _ = run(tmp_path, unsorted_input(False), sort_reads=True)
    check(bam, bai, [WHOLE, (2, 0, 1 << 29)])
    assert R.parse_bai(bai)["n_no_coor"] == 3


# ---- refusals ----

OK3 = [G.short(b"a", b"chr1", 100), G.short(b"b", b"chr1", 200), G.short(b"c", b"chr3", 50)]
REFUSALS = {
    "start": (OK3[:2] + [G.short(b"x", b"chr1", 150)], _capi.UNSORTED, 2),
    "refid": (OK3 + [G.short(b"x", b"chr1", 900)], _capi.UNSORTED, 3),
    "placed_after_unplaced": (OK3 + [G.short(b"u", b"*", 0, flag=4, cigar=b"*"), G.short(b"x", b"chr3", 60)],
                              _capi.UNSORTED, 4),
    "limit": (OK3[:2] + [G.short(b"x", b"chr1", (1 << 29) - 10)], _capi.UNSUPPORTED, 2),
}


def refused(tmp_path, text: bytes, status: int, read: int, **kw):
    """neither file appears, and a pair that was there is untouched"""
    src = tmp_path / "in.sam"
    src.write_bytes(text)
    out = tmp_path / "out.bam"
    for keep in (False, True):
        if keep:
            out.write_bytes(b"old bam")
            (tmp_path / "out.bam.bai").write_bytes(b"old bai")
        with pytest.raises(_capi.BQSRError) as e:
            transform(str(src), str(out), bam_index=True, overwrite=keep, **kw)
        assert (e.value.status, e.value.read) == (status, read), str(e.value)
        left = sorted(os.listdir(str(tmp_path)))
        assert left == (["in.sam", "out.bam", "out.bam.bai"] if keep else ["in.sam"])
    assert out.read_bytes() == b"old bam" and (tmp_path / "out.bam.bai").read_bytes() == b"old bai"


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_name_the_read(tmp_path, name):
    recs, status, read = REFUSALS[name]
    refused(tmp_path, G.HEAD + b"".join(recs), status, read)


def test_refusal_in_a_later_partition(tmp_path):
    lines = G.lines(G.chunk_runs())
    lines.insert(4000, G.short(b"x", b"chr1", 7))  # far behind its neighbours
    text = G.HEAD + b"".join(lines)
    refused(tmp_path, text, _capi.UNSORTED, 4000, mark_duplicates=True, partition_bytes=len(text) // 5)


def test_end_at_the_limit_is_indexed(tmp_path):
    bam, bai, _ = run(tmp_path, G.HEAD + G.short(b"x", b"chr1", (1 << 29) - 29))
    check(bam, bai, [WHOLE, (0, (1 << 29) - 1, 1 << 29)])
    assert len(R.parse_bai(bai)["refs"][0]["linear"]) == 1 << 15


def test_sort_reads_with_a_placed_unmapped_read_is_refused(tmp_path):
    src = tmp_path / "in.sam"
    src.write_bytes(unsorted_input(True))
    with pytest.raises(_capi.BQSRError) as e:
        transform(str(src), str(tmp_path / "out.bam"), bam_index=True, sort_reads=True)
    # the 300 mapped reads, then the unmapped ones in the reverse of their input order: u2 u1 u0 pu
    assert e.value.status == _capi.UNSORTED and e.value.read == 303
    assert sorted(os.listdir(str(tmp_path))) == ["in.sam"]


# ---- without the flag ----

def test_without_the_flag_nothing_changes(tmp_path):
    text = G.long_reads(120)
    src = tmp_path / "in.sam"
    src.write_bytes(text)
    plain, indexed = str(tmp_path / "plain.bam"), str(tmp_path / "indexed.bam")
    st = transform(str(src), plain, bam_piece_reads=50)
    assert main([str(src), indexed, "-bam_index"]) == 0 and os.path.exists(indexed + ".bai")
    with open(plain, "rb") as fh:
        data = fh.read()
    assert file_stream(data) == B.stream(text)  # what the encoder's yardstick gives, members checked
    assert not os.path.exists(plain + ".bai") and not any(k.startswith("index") for k in st["bam"])
    transform(str(src), indexed, bam_piece_reads=50, bam_index=True, overwrite=True)
    with open(indexed, "rb") as fh:
        assert fh.read() == data  # the index changes no byte of the BAM
