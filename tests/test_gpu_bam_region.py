"""`python -m adam_amd.bam_index` and `-region` on the device
(adam_amd/csrc/bam_windows.hip, adam_amd/bam_index.py, inputs.SamInput) against
tests/_bai_ref.py: the index bytes of BAMs under chosen member cuts
(tests/_bgzf_pack.py) and window sizes, the refusals, the records a region
read parses, and the commands' output on a region against the same command on
a SAM file of the region's lines."""
import os

import pytest

import _bai_gen as G
import _bai_ref as R
import _bam_ref as B
import _bgzf_pack as K
import _mpileup_gen as MG
from adam_amd import _capi, bam_index as BI, bqsr, inputs, synth
from adam_amd.samgen import sam_text
from adam_amd.sam import SamText

pytestmark = pytest.mark.gpu

STRADDLERS = ("long_reads", "exact_member_then_more", "exact_member_last")

_bais = {}


def own_index(shape, cut):
    if (shape, cut) not in _bais:
        _bais[shape, cut] = R.bai_of_bam(K.bam_file(shape, cut))
    return _bais[shape, cut]


def index_of(tmp_path, bam: bytes, piece=None, name="in.bam"):
    path = tmp_path / name
    path.write_bytes(bam)
    st = BI.bam_index(str(path), overwrite=True, piece_bytes=piece)
    assert sorted(os.listdir(str(tmp_path))) == [name, name + ".bai"] and st["output"] == str(path) + ".bai"
    return (tmp_path / (name + ".bai")).read_bytes(), st


# ---- the index ----

@pytest.mark.parametrize("cut", ["project", "small"])
@pytest.mark.parametrize("shape", sorted(K.SHAPES))
def test_index_bytes(tmp_path, shape, cut):
    bam = K.bam_file(shape, cut)
    bai, st = index_of(tmp_path, bam)
    assert bai == own_index(shape, cut)
    assert st["windows_host"] == 0 and st["reads"] == len(G.lines(K.text_of(shape)))  # the device chain ran
    assert st["members_host"] == 0  # and the device inflate, for every member
    assert st["members_total"] == len(R.Stream(bam).raw) and st["index_bytes"] == len(bai)


@pytest.mark.parametrize("cut", sorted(K.CUTS))
@pytest.mark.parametrize("shape", STRADDLERS)
def test_index_bytes_under_every_cut_and_piece(tmp_path, shape, cut):
    bam = K.bam_file(shape, cut)
    for piece in K.PIECES:
        bai, st = index_of(tmp_path, bam, piece)
        assert bai == own_index(shape, cut), piece
        assert st["windows_host"] == 0 and st["windows_device"] >= (2 if piece and shape == "long_reads" else 1), piece
        assert st["members_host"] == 0, piece
        if piece == 3000 and shape == "long_reads" and cut == "small":
            assert st["windows_device"] > 200  # a window per record or two (elsewhere a member is a window)


def test_index_of_the_project_s_own_output(tmp_path):
    from adam_amd.transform import transform
    src = tmp_path / "in.sam"
    src.write_bytes(G.chunk_runs())
    out = str(tmp_path / "out.bam")
    transform(str(src), out, bam_index=True)
    with open(out + ".bai", "rb") as fh:
        theirs = fh.read()
    st = BI.bam_index(out, out=str(tmp_path / "again.bai"))
    assert (tmp_path / "again.bai").read_bytes() == theirs and st["windows_host"] == 0
    assert BI.main([out, "-output", str(tmp_path / "cli.bai"), "-piece_bytes", "100000"]) == 0
    assert (tmp_path / "cli.bai").read_bytes() == theirs
    assert BI.main([out]) == 2 and BI.main([out, "-overwrite"]) == 0  # OUT.bam.bai is there already


def decoy_bam():
    """(file, text): a record whose QUAL bytes spell two plausible BAM records (block_size 33, refID 0, pos 0, a
    one-byte name), with a member cut exactly where they start: that member's guess is not on the chain, so the
    device check declines and the window is walked by the host"""
    fake = bytes([33, 0, 0, 0] + [0] * 8 + [1] + [0] * 24)
    assert len(fake) == 37
    qual = bytes(33 + b for b in fake * 2) + b"I" * 26
    text = (G.HEAD + b"".join(G.short(b"a%d" % i, b"chr1", 1000 + i) for i in range(100))
            + G.rec(b"decoy", 0, b"chr1", 1100, b"100M", b"A" * 100, qual)
            + b"".join(G.short(b"b%d" % i, b"chr1", 1101 + i) for i in range(100)))
    recs, stream = B.records(text), B.stream(text)
    cut = len(B.header(text)[0]) + sum(len(r) for r in recs[:100]) + 36 + len(b"decoy\0") + 4 + 50
    assert stream[cut:cut + 74] == fake * 2
    return K.member(stream[:cut]) + K.member(stream[cut:]) + K.EOF, text


def test_host_walk_where_the_device_check_declines(tmp_path):
    bam, text = decoy_bam()
    bai, st = index_of(tmp_path, bam)
    assert bai == R.bai_of_bam(bam) and (st["windows_device"], st["windows_host"]) == (0, 1) and st["reads"] == 201
    region = (0, 1090, 1120)
    got, st = region_lines(bam, bai, region, None)
    assert G.lines(got) == [G.lines(text)[i] for i in R.scan(bam, *region)] and st["windows_host"] >= 1
    assert any(l.startswith(b"decoy\t") for l in G.lines(got))


# ---- refusals ----

OK3 = [G.short(b"a", b"chr1", 100), G.short(b"b", b"chr1", 200), G.short(b"c", b"chr3", 50)]
UNSORTED = {
    "start": OK3[:2] + [G.short(b"x", b"chr1", 150)],
    "refid": OK3 + [G.short(b"x", b"chr1", 900)],
    "placed_after_unplaced": OK3 + [G.short(b"u", b"*", 0, flag=4, cigar=b"*"), G.short(b"x", b"chr3", 60)],
    "limit": OK3[:2] + [G.short(b"x", b"chr1", (1 << 29) - 10)],
    "late": G.lines(G.chunk_runs())[:4000] + [G.short(b"x", b"chr1", 7)] + G.lines(G.chunk_runs())[4000:],
}


def packed(text: bytes, cut="small") -> bytes:
    head = B.header(text)[0]
    ends, p = [len(head)], len(head)
    for r in B.records(text):
        p += len(r)
        ends.append(p)
    return K.pack(B.stream(text), ends, cut)


def refused(tmp_path, bam: bytes, status: str, read, piece=None):
    """no file appears, and an index that was there stays, with and without -overwrite"""
    path = tmp_path / "in.bam"
    path.write_bytes(bam)
    with pytest.raises(_capi.BQSRError) as e:
        BI.bam_index(str(path), piece_bytes=piece)
    assert e.value.name == status and (read is None or e.value.read == read), str(e.value)
    assert sorted(os.listdir(str(tmp_path))) == ["in.bam"]
    (tmp_path / "in.bam.bai").write_bytes(b"old bai")
    with pytest.raises(FileExistsError):
        BI.bam_index(str(path), piece_bytes=piece)
    with pytest.raises(_capi.BQSRError):
        BI.bam_index(str(path), overwrite=True, piece_bytes=piece)
    assert sorted(os.listdir(str(tmp_path))) == ["in.bam", "in.bam.bai"]
    assert (tmp_path / "in.bam.bai").read_bytes() == b"old bai"


@pytest.mark.parametrize("name", sorted(UNSORTED))
def test_refusals_of_the_yardstick(tmp_path, name):
    bam = packed(G.HEAD + b"".join(UNSORTED[name]))
    with pytest.raises(R.BaiRefusal) as want:
        R.bai_of_bam(bam)
    assert want.value.status == ("UNSUPPORTED" if name == "limit" else "UNSORTED")
    refused(tmp_path, bam, want.value.status, want.value.read, 70000 if name == "late" else None)


def test_file_cut_inside_a_member(tmp_path):
    bam = K.bam_file("chunk_runs", "stored")[:-28]
    refused(tmp_path, bam[:-1000], "SAM_PARSE", None)


def test_file_cut_inside_a_record(tmp_path):
    text = G.chunk_runs()
    stream = B.stream(text)
    n = 5000
    cut = len(B.header(text)[0]) + sum(len(r) for r in B.records(text)[:n]) + 50  # 50 bytes into record 5000
    for piece in (None, 3000):
        refused(tmp_path, K.pack(stream[:cut], [], "small"), "SAM_PARSE", n, piece)
        os.remove(str(tmp_path / "in.bam.bai"))
    refused(tmp_path, K.pack(stream[:cut - 48], [], "project"), "SAM_PARSE", n)  # its size word cut in two


def test_size_word_that_points_past_the_file(tmp_path):
    """refused from the stream's remaining length: the reader does not inflate the rest of the file for it"""
    text = G.chunk_runs()
    stream = bytearray(B.stream(text))
    n = 5000
    at = len(B.header(text)[0]) + sum(len(r) for r in B.records(text)[:n])
    stream[at:at + 4] = (0x7FFFFFFF).to_bytes(4, "little")
    for piece in (3000, None):
        refused(tmp_path, K.pack(bytes(stream), [], "small"), "SAM_PARSE", n, piece)
        os.remove(str(tmp_path / "in.bam.bai"))


def test_malformed_record_after_the_region_s_chunk(tmp_path):
    """a record at the chunk's v whose CIGAR count overruns its block_size: the region read does not take it and
    is not failed by it; an index of the whole file is refused naming it.  Stored members keep every virtual
    offset of the undamaged file, whose index is used."""
    text = (G.HEAD + b"".join(G.short(b"a%d" % i, b"chr1", 1000 + i) for i in range(100))
            + b"".join(G.short(b"b%d" % i, b"chr1", (1 << 20) + 1 + i) for i in range(100)))
    good = packed(text, "stored")
    stream = bytearray(B.stream(text))
    at = len(B.header(text)[0]) + sum(len(r) for r in B.records(text)[:100])
    stream[at + 16:at + 18] = b"\xff\xff"  # n_cigar_op of record 100
    bad = K.pack(bytes(stream), [], "stored")
    assert len(bad) == len(good)
    bai = R.bai_of_bam(good)
    region = (0, 999, 1200)
    got, st = region_lines(bad, bai, region, None)
    assert G.lines(got) == G.lines(text)[:100] and st["records_seen"] > 100  # (record 100 was in the window)
    refused(tmp_path, bad, "SAM_PARSE", 100)


def test_not_a_bam(tmp_path):
    refused(tmp_path, K.member(b"BAX\1" + bytes(40)) + K.EOF, "SAM_PARSE", None)
    os.remove(str(tmp_path / "in.bam.bai"))
    refused(tmp_path, G.chunk_runs(), "SAM_PARSE", None)


def test_no_eof_marker_and_a_full_last_member(tmp_path):
    text = K.text_of("long_reads")
    stream = B.stream(text)
    parts = K.by_size(60000)(stream[:-65536], []) + [stream[-65536:]]
    refused(tmp_path, b"".join(K.member(p) for p in parts), "UNSUPPORTED", None)
    os.remove(str(tmp_path / "in.bam.bai"))
    bam = b"".join(K.member(p) for p in parts) + K.EOF  # with the marker the same members are indexed
    assert index_of(tmp_path, bam)[0] == R.bai_of_bam(bam)


# ---- a region's records ----

_full, _scans = {}, {}


def full_lines(shape):
    """the lines of the whole file's parse (made once per shape: they do not depend on the cut)"""
    if shape not in _full:
        sam = SamText(K.bam_file(shape, "project"), bam=True)
        try:
            _full[shape] = G.lines(sam.text())
        finally:
            sam.close()
        assert len(_full[shape]) == len(G.lines(K.text_of(shape)))
    return _full[shape]


def scan(shape, region):
    if (shape, region) not in _scans:
        _scans[shape, region] = R.scan(K.bam_file(shape, "project"), *region)
    return _scans[shape, region]


def region_lines(bam: bytes, bai: bytes, region, piece):
    sam, st = BI.region_text(bam, bqsr.Context.get(0), BI.BaiIndex(bai), *region, piece_bytes=piece)
    try:
        text = sam.text()
        assert sam.counts().n_reads == st["records_kept"]
        assert sam.bam_form == (2 if st["members_host"] == 0 else 1)
    finally:
        sam.close()
    return text, st


@pytest.mark.parametrize("cut", sorted(K.CUTS))
@pytest.mark.parametrize("shape", sorted(K.SHAPES))
def test_region_parse(shape, cut):
    bam = K.bam_file(shape, cut)
    want_all = full_lines(shape)
    head = K.text_of(shape)[:len(K.text_of(shape)) - sum(len(l) for l in G.lines(K.text_of(shape)))]
    indexes = [own_index(shape, cut), K.coarse(own_index(shape, cut)), K.no_linear(own_index(shape, cut))]
    for piece in K.PIECES:
        for bai in indexes:
            for region in G.REGIONS:
                text, st = region_lines(bam, bai, region, piece)
                want = [want_all[i] for i in scan(shape, region)]
                assert G.lines(text) == want, (piece, indexes.index(bai), region)
                assert text == head + b"".join(want)
                assert st["windows_host"] == 0 and st["records_kept"] == len(want) <= st["records_seen"]
                assert st["members_host"] == 0
                assert st["members_read"] <= 3 * st["members_total"] + 3


def test_narrow_region_reads_few_members(tmp_path):
    bam = K.bam_file("chunk_runs", "small")
    path = tmp_path / "in.bam"
    path.write_bytes(bam)
    (tmp_path / "in.bam.bai").write_bytes(own_index("chunk_runs", "small"))
    with inputs.SamInput(str(path), bqsr.Context.get(0), inputs.Phases(), 1000, region="chr1:163841-163940") as src:
        assert src.bam and src.n_partitions == 1
        got = [(G.lines(sam.text()), base) for sam, base in src]
        st = src.region_stats
    want = [full_lines("chunk_runs")[i] for i in R.scan(bam, 0, 163840, 163940)]
    assert got == [(want, 0)] and len(want) > 0
    assert st["members_read"] < st["members_total"] / 2 and st["records_kept"] == len(want)
    assert st["records_seen"] < len(full_lines("chunk_runs")) / 2


# ---- the commands ----

def region_files(tmp_path, text: bytes, region, cut="small"):
    """IN.bam (+ .bai) of `text`, and region.sam: the header plus the lines of the records _bai_ref.scan names"""
    bam = packed(text, cut)
    (tmp_path / "in.bam").write_bytes(bam)
    (tmp_path / "in.bam.bai").write_bytes(R.bai_of_bam(bam))
    lines = G.lines(text)
    keep = R.scan(bam, *region)
    assert 0 < len(keep) < len(lines)
    head = text[:len(text) - sum(len(l) for l in lines)]
    (tmp_path / "region.sam").write_bytes(head + b"".join(lines[i] for i in keep))
    return str(tmp_path / "in.bam"), str(tmp_path / "region.sam")


def pileup_text():
    """sorted, conflict-free reads of one reference per contig (tests/_mpileup_gen.py)"""
    specs = [(1000 + 7 * i, ("40M", "10M2D30M", "5S20M3I15M", "20M100N20M")[i % 4], dict(rname="c1")) for i in range(300)]
    specs += [(500 + 11 * i, "30M", dict(rname="c2")) for i in range(100)]
    return MG.sam_text(specs, seed=11)


PILEUP_REGION, PILEUP_ARG = (0, 1999, 2600), "c1:2000-2600"


def stdout_of(main, argv, capsys):
    capsys.readouterr()
    assert main(argv) == 0
    return capsys.readouterr().out


def test_flagstat_on_a_region(tmp_path, capsys):
    from adam_amd.flagstat import main
    text = G.sort_text(sam_text(synth.generate(2000, lens=(100,), n_rg=2, seed=15, p_q2tail=0.0), n_rg=2))
    rid, beg, end = pick_region(text)
    bam, sam = region_files(tmp_path, text, (rid, beg, end))
    arg = "%s:%d-%d" % (ref_name(text, rid), beg + 1, end)
    assert stdout_of(main, [bam, "-region", arg], capsys) == stdout_of(main, [sam], capsys)
    os.rename(bam + ".bai", str(tmp_path / "elsewhere.bai"))
    assert stdout_of(main, [bam, "-region", arg, "-bai", str(tmp_path / "elsewhere.bai")], capsys) == \
        stdout_of(main, [sam], capsys)


def ref_name(text: bytes, rid: int) -> str:
    return [l.split(b"\t")[1][3:] for l in text.split(b"\n") if l.startswith(b"@SQ")][rid].decode()


def pick_region(text: bytes):
    """(refID, beg, end) around the middle third of the reads of the reference with the most reads"""
    names = [l.split(b"\t")[1][3:] for l in text.split(b"\n") if l.startswith(b"@SQ")]
    by_ref = {}
    for l in G.lines(text):
        f = l.split(b"\t")
        if f[2] in names and int(f[3]) > 0:
            by_ref.setdefault(f[2], []).append(int(f[3]) - 1)
    name = max(by_ref, key=lambda k: len(by_ref[k]))
    pos = sorted(by_ref[name])
    return names.index(name), pos[len(pos) // 3], pos[2 * len(pos) // 3] + 1


def test_mpileup_on_a_region(tmp_path):
    from adam_amd.mpileup import main
    bam, sam = region_files(tmp_path, pileup_text(), PILEUP_REGION)
    a, b = str(tmp_path / "a.txt"), str(tmp_path / "b.txt")
    assert main([bam, "-output", a, "-region", PILEUP_ARG]) == 0 and main([sam, "-output", b]) == 0
    with open(a, "rb") as fa, open(b, "rb") as fb:
        got = fa.read()
        assert got == fb.read() and len(got) > 1000


def test_transform_markdup_and_bqsr_on_a_region(tmp_path):
    from adam_amd.transform import main
    text = G.sort_text(sam_text(synth.generate(2000, lens=(100,), n_rg=2, seed=15, p_q2tail=0.0), n_rg=2))
    rid, beg, end = pick_region(text)
    bam, sam = region_files(tmp_path, text, (rid, beg, end))
    arg = "%s:%d-%d" % (ref_name(text, rid), beg + 1, end)
    a, b = str(tmp_path / "a.sam"), str(tmp_path / "b.sam")
    steps = ["-mark_duplicate_reads", "-recalibrate_base_qualities"]
    assert main([bam, a] + steps + ["-region", arg]) == 0 and main([sam, b] + steps) == 0
    with open(a, "rb") as fa, open(b, "rb") as fb:
        got = fa.read()
        assert got == fb.read() and len(G.lines(got)) == len(G.lines(open(sam, "rb").read()))


def test_print_tags_and_realignment_targets_on_a_region(tmp_path, capsys):
    from adam_amd.print_tags import main as print_tags
    from adam_amd.realignment_targets import main as targets
    bam, sam = region_files(tmp_path, pileup_text(), PILEUP_REGION)
    for main, more in ((print_tags, ["-count", "NM", "-list", "5"]), (targets, [])):
        assert stdout_of(main, [bam, "-region", PILEUP_ARG] + more, capsys) == stdout_of(main, [sam] + more, capsys)


def test_reads2ref_and_aggregate_pileups_on_a_region(tmp_path):
    from adam_amd import parquet as P
    from adam_amd.aggregate_pileups import main as aggregate
    from adam_amd.reads2ref import main as reads2ref
    bam, sam = region_files(tmp_path, pileup_text(), PILEUP_REGION)
    for k, main in enumerate((reads2ref, aggregate)):
        a, b = str(tmp_path / ("a%d.adam" % k)), str(tmp_path / ("b%d.adam" % k))
        assert main([bam, a, "-region", PILEUP_ARG]) == 0 and main([sam, b]) == 0
        ta, tb = P.read_table(a), P.read_table(b)
        assert ta.num_rows > 100 and ta.equals(tb)
