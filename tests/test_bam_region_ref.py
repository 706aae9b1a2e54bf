"""adam_amd.bam_index without a device: the region syntax, the .bai reader
against tests/_bai_ref.py, the merged chunk list a region read follows (on the
project's own index and on three altered ones), and the refusals that come
before anything is read or created.  The BAM files are those of the GPU tests
(tests/_bgzf_pack.py), and ``_bai_ref.query == _bai_ref.scan`` is pinned on
them."""
import os

import pytest

import _bai_gen as G
import _bai_ref as R
import _bgzf_pack as K
from adam_amd import _capi, bam_index as BI, inputs

NAMES = ["chr1", "chr2", "chr3", "HLA-A*01:01", "HLA-A*01:01:5", "7"]


@pytest.mark.parametrize("text,want", [
    ("chr1", (0, 0, 1 << 29)),
    ("chr2:100", (1, 99, 1 << 29)),
    ("chr3:100-200", (2, 99, 200)),
    ("chr1:1-1", (0, 0, 1)),
    ("chr1:5-999999999999", (0, 4, 1 << 29)),     # END clamped
    ("chr1:536870912", (0, (1 << 29) - 1, 1 << 29)),
    ("HLA-A*01:01", (3, 0, 1 << 29)),             # the whole string is a name first
    ("HLA-A*01:01:5", (4, 0, 1 << 29)),           # (not HLA-A*01:01 from 5)
    ("HLA-A*01:01:7-9", (3, 6, 9)),
    ("HLA-A*01:01:5:7-9", (4, 6, 9)),
    ("7:7", (5, 6, 1 << 29)),
])
def test_region_forms(text, want):
    assert BI.parse_region(text, NAMES) == want


@pytest.mark.parametrize("text", ["*", "chrX", "chrX:1-2", "chr1:", "chr1:0-5", "chr1:9-8", "chr1:-5", "chr1:1-",
                                  "chr1:1,000-2,000", "chr1:+1-5", "chr1:1-5-9", "chr1:a-b", "chr1: 1-2", "",
                                  "chr1:536870913", "chr1:١-5"])
def test_region_refusals(text):
    with pytest.raises(ValueError):
        BI.parse_region(text, NAMES)


# ---- the .bai reader ----

def own_index(shape, cut="project"):
    return R.bai_of_bam(K.bam_file(shape, cut))


@pytest.mark.parametrize("shape", sorted(K.SHAPES))
def test_bai_index_reads_what_parse_bai_reads(shape):
    bai = own_index(shape)
    P, X = R.parse_bai(bai), BI.BaiIndex(bai)
    assert X.n_ref == len(P["refs"]) and X.n_no_coor == P["n_no_coor"]
    for r, ref in enumerate(P["refs"]):
        assert X.linear[r] == ref["linear"]
        assert X.bins[r] == {b: list(c) for b, c in ref["bins"].items() if b != R.PSEUDO_BIN}
        assert X.meta[r] == (list(ref["bins"][R.PSEUDO_BIN]) if R.PSEUDO_BIN in ref["bins"] else None)
    X.validate(3, len(K.bam_file(shape, "project")))


def test_bai_index_refuses_what_does_not_parse():
    bai = own_index("references")
    size = len(K.bam_file("references", "project"))
    for bad in (b"", b"BAM\1" + bai[4:], bai[:-9], bai[:40], bai + b"\0", bai[:8] + b"\xff\xff\xff\xff" + bai[12:]):
        with pytest.raises(ValueError):
            BI.BaiIndex(bad)
    assert BI.BaiIndex(bai[:-8]).n_no_coor is None  # (n_no_coor is optional)
    X = BI.BaiIndex(bai)
    with pytest.raises(ValueError, match="references"):
        X.validate(2, size)
    with pytest.raises(ValueError, match="outside the file"):
        X.validate(3, 0)


# ---- the chunk list ----

_walks = {}


def walked(shape, cut):
    key = (shape, cut)
    if key not in _walks:
        S, _, recs = R.walk(K.bam_file(shape, cut))
        _walks[key] = (S, recs, {r[4]: i for i, r in enumerate(recs)})
    return _walks[key]


def reached(shape, cut, bai, rid, beg, end):
    """the ordinals of the records a reader of index.chunks() passes, in the order it passes them"""
    S, recs, ordinal = walked(shape, cut)
    out = []
    for u, v in BI.BaiIndex(bai).chunks(rid, beg, end):
        i = ordinal[u]  # (a chunk starts on a record)
        while i < len(recs) and recs[i][4] < v:
            out.append(i)
            i += 1
    return out


def covers(shape, cut, bai):
    bam = K.bam_file(shape, cut)
    for rid, beg, end in G.REGIONS:
        got = reached(shape, cut, bai, rid, beg, end)
        assert len(set(got)) == len(got) and got == sorted(got), (rid, beg, end)  # each record once, in file order
        assert set(R.scan(bam, rid, beg, end)) <= set(got), (rid, beg, end)


@pytest.mark.parametrize("cut", sorted(K.CUTS))
@pytest.mark.parametrize("shape", sorted(K.SHAPES))
def test_chunks_reach_every_overlapping_record_once(shape, cut):
    covers(shape, cut, own_index(shape, cut))


@pytest.mark.parametrize("how", sorted(K.ALTERED))
@pytest.mark.parametrize("cut", sorted(K.CUTS))
@pytest.mark.parametrize("shape", sorted(K.SHAPES))
def test_chunks_of_altered_indexes(shape, cut, how):
    covers(shape, cut, K.ALTERED[how](own_index(shape, cut)))


def test_altered_indexes_are_what_they_say():
    bai = own_index("chunk_runs", "small")
    P = R.parse_bai(bai)
    assert max(len(c) for c in P["refs"][0]["bins"].values()) > 2
    C = BI.BaiIndex(K.coarse(bai))
    assert all(len(c) == 1 for c in C.bins[0].values())
    assert BI.BaiIndex(K.no_linear(bai)).linear == [[], [], []]
    F = BI.BaiIndex(K.folded(bai))
    assert F.bins[0] and all(b < 4681 for b in F.bins[0]) and F.meta[0] is not None


@pytest.mark.parametrize("cut", sorted(K.CUTS))
@pytest.mark.parametrize("shape", sorted(K.SHAPES))
def test_yardstick_query_is_scan_on_these_files(shape, cut):
    bam = K.bam_file(shape, cut)
    bai = R.bai_of_bam(bam)
    for rid, beg, end in G.REGIONS:
        assert R.query(bam, bai, rid, beg, end) == R.scan(bam, rid, beg, end), (rid, beg, end)


def test_member_cuts_are_what_they_say():
    S = R.Stream(K.bam_file("long_reads", "small"))
    _, _, recs = R.walk(K.bam_file("long_reads", "small"))
    starts = {r[4] >> 16 for r in recs}
    assert max(len(r) for r in S.raw) == 1000 and len(starts) < len(S.raw) / 2  # most members hold no record start
    S = R.Stream(K.bam_file("chunk_runs", "empty_member"))
    assert 0 in [len(r) for r in S.raw[1:-2]]
    assert K.bam_file("chunk_runs", "no_eof")[-28:] != K.EOF and K.bam_file("chunk_runs", "stored")[-28:] == K.EOF
    assert len(R.Stream(K.bam_file("long_header", "small")).raw[0]) == 1000 and len(K.LONG_HEADER) > 4000
    S, _, recs = R.walk(K.bam_file("chunk_runs", "records"))
    assert len(S.raw) > 10 and set(S.start[1:]) <= {S.pos(r[4]) for r in recs} | {len(S.data)}  # cut on record ends


def test_narrow_region_names_few_members():
    """the input's side of the GPU test's members_read bound"""
    bam = K.bam_file("chunk_runs", "small")
    S = R.Stream(bam)
    ref = R.parse_bai(R.bai_of_bam(bam))["refs"][0]  # the chunks _bai_ref names, as _bai_ref.query takes them
    low = ref["linear"][163840 >> 14]
    chunks = [c for b in R.reg2bins(163840, 163940) for c in ref["bins"].get(b, ()) if c[1] > low]
    named = set()
    for u, v in chunks:
        named |= set(range(S.member_of[u >> 16], S.member_of[v >> 16] + 1))
    assert chunks and len(named) < len(S.raw) / 2
    assert len(R.scan(bam, 0, 163840, 163940)) > 0


# ---- the refusals before anything is read or created ----

@pytest.fixture
def no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the native library was loaded")
    monkeypatch.setattr(_capi, "lib", boom)


def files(tmp_path):
    bam = tmp_path / "in.bam"
    bam.write_bytes(K.bam_file("references", "project"))
    sam = tmp_path / "in.sam"
    sam.write_bytes(K.text_of("references"))
    return str(bam), str(sam)


def test_early_refusals(tmp_path, no_device):
    bam, sam = files(tmp_path)
    before = sorted(os.listdir(str(tmp_path)))
    with pytest.raises(ValueError, match="not a BAM"):
        inputs.region_plan(sam, "chr1")
    adam = tmp_path / "reads.adam"
    adam.mkdir()
    with pytest.raises(ValueError, match="Parquet"):
        inputs.region_plan(str(adam), "chr1")
    adam.rmdir()
    with pytest.raises(ValueError, match="python -m adam_amd.bam_index"):
        inputs.region_plan(bam, "chr1")
    with pytest.raises(ValueError, match="no index file"):
        inputs.region_plan(bam, "chr1", str(tmp_path / "other.bai"))
    with pytest.raises(ValueError, match="-bai goes with -region"):
        inputs.region_plan(bam, None, "x.bai")
    assert sorted(os.listdir(str(tmp_path))) == before
    (tmp_path / "in.bam.bai").write_bytes(R.bai_of_bam(K.bam_file("references", "project")))
    for region in ("chrX", "chrX:1-5", "*", "chr1:0-5", "chr1:9-8"):
        with pytest.raises(ValueError):
            inputs.region_plan(bam, region)
        with pytest.raises(ValueError):
            with inputs.SamInput(bam, None, inputs.Phases(), region=region):
                pass
    index, rid, beg, end = inputs.region_plan(bam, "chr3:1-100")
    assert (rid, beg, end) == (2, 0, 100) and index.n_ref == 3
    assert inputs.region_plan(bam, None) is None
    # IN.bai is found too, and an index of another file is refused
    os.rename(str(tmp_path / "in.bam.bai"), str(tmp_path / "in.bai"))
    assert inputs.region_plan(bam, "chr1")[1:] == (0, 0, 1 << 29)
    (tmp_path / "in.bai").write_bytes(b"BAI\1" + bytes(4) + bytes(8))
    with pytest.raises(ValueError, match="references"):
        inputs.region_plan(bam, "chr1")
    assert sorted(os.listdir(str(tmp_path))) == sorted(before + ["in.bai"])


def test_the_plan_is_made_once(tmp_path, no_device, monkeypatch):
    bam, _ = files(tmp_path)
    (tmp_path / "in.bam.bai").write_bytes(R.bai_of_bam(K.bam_file("references", "project")))
    plan = inputs.region_plan(bam, "chr1:1-100")
    assert isinstance(plan, inputs.RegionPlan) and plan[1:] == (0, 0, 100)

    def again(*a, **k):
        raise AssertionError("the header was read a second time")
    monkeypatch.setattr(BI, "bam_header", again)
    monkeypatch.setattr(BI.BaiIndex, "read", again)
    assert inputs.region_plan(bam, plan) is plan and inputs.region_plan(bam, plan, "other.bai") is plan
    with inputs.SamInput(bam, None, inputs.Phases(), region=plan) as src:
        assert src.plan is plan and src.n_partitions == 1


def test_a_header_that_does_not_inflate_is_refused_early(tmp_path, no_device):
    from adam_amd.flagstat import main
    bam, _ = files(tmp_path)
    (tmp_path / "in.bam.bai").write_bytes(R.bai_of_bam(K.bam_file("references", "project")))
    data = bytearray(K.bam_file("references", "project"))
    data[18:30] = b"\xff" * 12  # the first member's DEFLATE data
    (tmp_path / "in.bam").write_bytes(bytes(data))
    with pytest.raises(ValueError, match="does not inflate"):
        inputs.region_plan(bam, "chr1")
    with pytest.raises(SystemExit) as e:
        main([bam, "-region", "chr1"])
    assert e.value.code == 2


def test_help_says_what_a_region_means_for_mates(capsys):
    from adam_amd.transform import main
    with pytest.raises(SystemExit):
        main(["-h"])
    text = " ".join(capsys.readouterr().out.split())
    assert "MarkDuplicates and BQSR" in text and "a mate outside the region is absent" in text


COMMANDS = ["flagstat", "print_tags", "mpileup", "reads2ref", "aggregate_pileups", "realignment_targets", "transform"]


@pytest.mark.parametrize("command", COMMANDS)
def test_commands_refuse_early_with_exit_2(tmp_path, no_device, command, capsys):
    import importlib
    bam, sam = files(tmp_path)
    main = importlib.import_module("adam_amd." + command).main
    out = [str(tmp_path / "out.sam")] if command in ("transform", "reads2ref", "aggregate_pileups") else []
    before = sorted(os.listdir(str(tmp_path)))
    for argv in ([sam] + out + ["-region", "chr1"],          # SAM input
                 [bam] + out + ["-region", "chr1"],          # no index
                 [bam] + out + ["-region", "chr1", "-bai", str(tmp_path / "none.bai")]):
        with pytest.raises(SystemExit) as e:
            main(argv)
        assert e.value.code == 2
        assert sorted(os.listdir(str(tmp_path))) == before
    assert "python -m adam_amd.bam_index" in capsys.readouterr().err
    (tmp_path / "in.bam.bai").write_bytes(R.bai_of_bam(K.bam_file("references", "project")))
    with pytest.raises(SystemExit) as e:
        main([bam] + out + ["-region", "chrX:5"])             # unknown reference
    assert e.value.code == 2 and sorted(os.listdir(str(tmp_path))) == sorted(before + ["in.bam.bai"])


def test_bam_index_refuses_before_the_device(tmp_path, no_device):
    bam, sam = files(tmp_path)
    (tmp_path / "in.bam.bai").write_bytes(b"old")
    with pytest.raises(FileExistsError):
        BI.bam_index(bam)
    assert BI.main([bam]) == 2 and (tmp_path / "in.bam.bai").read_bytes() == b"old"
    with pytest.raises(ValueError):
        BI.bam_index(bam, overwrite=True, piece_bytes=0)
    with pytest.raises(_capi.BQSRError, match="not a BAM"):
        BI.bam_index(sam)
    assert sorted(os.listdir(str(tmp_path))) == ["in.bam", "in.bam.bai", "in.sam"]


def test_symbols_are_declared_and_exported():
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "adam_sam.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    declared = set(re.findall(r"\b(bqsr_bam_reader_[a-z_]+|bqsr_bam_index_add_window)\s*\(", text))
    assert declared == set(BI.SYMBOLS) and declared <= set(_capi.EXPORTS)
