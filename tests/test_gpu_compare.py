"""`compare` / `findreads` on the device (csrc/compare.hip) against the host
path (compare.compare_host): exact equality of the four totals, of every key
and count of all five histograms, and of the findreads rows in order, on
seeded SAM pairs (tests/_compare_gen.py)."""
import random

import pytest

from _compare_gen import HDR, bucket_hash, fnv1a, gen_pair, rec
from adam_amd import _capi, compare as C

pytestmark = pytest.mark.gpu
ALL = C.COMPARISON_NAMES


def write_pair(tmp_path, sams, tag=""):
    p1, p2 = tmp_path / ("1%s.sam" % tag), tmp_path / ("2%s.sam" % tag)
    p1.write_bytes(sams[0])
    p2.write_bytes(sams[1])
    return str(p1), str(p2)


def same(dev, host):
    assert (dev.total1, dev.unique1, dev.total2, dev.unique2) == (host.total1, host.unique1, host.total2, host.unique2)
    assert set(dev.histograms) == set(host.histograms)
    for c in host.histograms:
        assert dev.histograms[c] == host.histograms[c], c


def check(p1, p2, e1="latin-1", e2="latin-1", **kw):
    host = C.compare_host(p1, p2, ALL, e1, e2)
    dev = C.compare_device(p1, p2, ALL, e1, e2, **kw)
    same(dev, host)
    return dev, host


def test_no_joined_pairs(tmp_path):
    p1, p2 = write_pair(tmp_path, gen_pair(1, 40, disjoint=True))
    dev, host = check(p1, p2)
    assert host.total1 == host.unique1 > 0 and host.total2 == host.unique2 > 0 and dev.stats["pairs"] == 0


def test_one_read(tmp_path):
    p1, p2 = write_pair(tmp_path, (HDR + rec(b"a", 16, b"IIJ"), HDR + rec(b"a", 16, b"IIK", pos=12)))
    dev, host = check(p1, p2)
    assert host.histograms["positions"] == {2: 1} and host.histograms["baseqs"] == {(40, 40): 2, (41, 42): 1}
    p1, p2 = write_pair(tmp_path, (HDR + rec(b"a", 16, b"I"), HDR), "e")  # an input without reads
    dev, host = check(p1, p2)
    assert (host.total1, host.unique1, host.total2) == (1, 1, 0)


@pytest.mark.parametrize("n_names", [63, 64, 65, 257])
def test_bucket_counts_around_a_wavefront(tmp_path, n_names):
    p1, p2 = write_pair(tmp_path, gen_pair(100 + n_names, n_names))
    check(p1, p2)


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """about 5 000 reads with one pair of 4 096-base reads; the host result computed once"""
    d = tmp_path_factory.mktemp("cmp")
    sams = gen_pair(7, 2300, long_pair=True)
    assert 4500 < sams[0].count(b"\n") < 6000
    p1, p2 = write_pair(d, sams)
    return p1, p2, C.compare_host(p1, p2, ALL)


def test_five_thousand_reads(big):
    p1, p2, host = big
    dev = C.compare_device(p1, p2, ALL)
    same(dev, host)
    assert dev.stats["pairs"] > 2000 and len(host.histograms["baseqs"]) > 500
    assert any(not (0 <= a < 64 and 0 <= b < 64) for a, b in host.histograms["baseqs"])
    assert host.histograms["overmatched"].get(False, 0) > 0 and len(host.histograms["mapqs"]) > 100


def test_flushes_between_chunks(big):
    # two workgroups share the chunks and flush their private tables before every chunk after the first
    p1, p2, host = big
    dev = C.compare_device(p1, p2, ALL, _flush_chars=16384, _groups=2)
    same(dev, host)
    assert dev.stats["baseq_chars"] > 4 * 16384 and dev.stats["flushes"] > 4


def test_every_comparison_alone(big):
    p1, p2, host = big
    for c in ALL:
        dev = C.compare_device(p1, p2, [c])
        assert dev.histograms == {c: host.histograms[c]}


def to_utf8(sam, seed):
    """the SAM with some QUAL chars replaced by 2-, 3- and 4-byte ones, written as UTF-8"""
    rng = random.Random(seed)
    out = []
    for line in sam.split(b"\n"):
        f = line.split(b"\t")
        if len(f) > 10 and not line.startswith(b"@"):
            s = ""
            for b in f[10]:
                u = rng.random()
                s += chr(b + 0x80) if u < 0.1 else "€" if u < 0.12 else "\U0001F600" if u < 0.13 else chr(b)
            f[10] = s.encode("utf-8")
        out.append(b"\t".join(f))
    return b"\n".join(out)


def test_utf8_side(tmp_path):
    s1, s2 = gen_pair(11, 300, wide=False)
    p1, p2 = write_pair(tmp_path, (s1, to_utf8(s2, 5)))
    dev, host = check(p1, p2, "latin-1", "utf-8")
    assert any(a < 0 or b < 0 for a, b in host.histograms["baseqs"])
    p1, p2 = write_pair(tmp_path, (to_utf8(s1, 6), to_utf8(s2, 5)), "u")
    check(p1, p2, "utf-8", "utf-8")
    p1, p2 = write_pair(tmp_path, (s1, HDR + rec(b"a", 16, b"I\xe9")), "bad")  # latin-1 bytes read as UTF-8
    with pytest.raises(_capi.BQSRError) as e:
        C.compare_device(p1, p2, ["baseqs"], "latin-1", "utf-8")
    assert e.value.status == _capi.SAM_PARSE and e.value.read == 0


def test_bad_utf8_leads_take_no_place(tmp_path):
    # bytes that are no UTF-8 leads (0xF5..0xFF), and a 4-byte lead before ASCII, in the last read of
    # the side: the decode gives them no place in the output (its slot is the read's byte count) and
    # the job fails with SAM_PARSE naming that read
    good = rec(b"a", 16, b"IIII") + rec(b"b", 16, "Ié€\U0001F600".encode("utf-8"))
    for k, tail in enumerate((bytes([0xFF] * 40 + [0xF8, 0xFB, 0xF5]) + b"\xf1AAA" + bytes([0xFE] * 20),
                              b"\xf1AAA",
                              bytes([0xFF, 0x49] * 2048),
                              bytes(range(0xF5, 0x100)) * 8)):
        p1, p2 = write_pair(tmp_path, (HDR + good + rec(b"z", 16, b"I" * len(tail)), HDR + good + rec(b"z", 16, tail)),
                            "t%d" % k)
        with pytest.raises(_capi.BQSRError) as e:
            C.compare_device(p1, p2, ["baseqs"], "latin-1", "utf-8")
        assert e.value.status == _capi.SAM_PARSE and e.value.read == 2 and "input 2" in str(e.value)
        with pytest.raises(_capi.BQSRError) as e:
            C.compare_device(p2, p1, ALL, "utf-8", "latin-1")
        assert e.value.status == _capi.SAM_PARSE and e.value.read == 2 and "input 1" in str(e.value)
        # the same bytes are fine as latin-1
        same(C.compare_device(p1, p2, ALL), C.compare_host(p1, p2, ALL))


def test_formats(tmp_path):
    # this build's own transform writes the same two inputs as BAM and as ADAM (a directory of part
    # files): every pairing gives the SAM result
    from adam_amd.transform import transform
    p1, p2 = write_pair(tmp_path, gen_pair(21, 200, wide=False))
    b1, b2 = str(tmp_path / "1.bam"), str(tmp_path / "2.bam")
    a1, a2 = str(tmp_path / "1.adam"), str(tmp_path / "2.adam")
    for src, dst in ((p1, b1), (p2, b2), (p1, a1), (p2, a2)):
        transform(src, dst)
    host = C.compare_host(p1, p2, ALL)
    for x, y in ((b1, a2), (a1, p2), (a1, a2), (b1, b2), (p1, b2), (b1, p2)):
        same(C.compare_device(x, y, ALL), host)
    for c in ALL:  # each comparison's own projection of the Parquet columns
        assert C.compare_device(a1, a2, [c]).histograms == {c: host.histograms[c]}
    f = "baseqs!=(40,40);mapqs=(60,60)"
    for x, y in ((b1, b2), (b1, a2), (a1, p2)):
        assert C.find_reads_device(x, y, "positions>0") == C.find_reads_host(p1, p2, "positions>0")
        assert C.find_reads_device(x, y, f) == C.find_reads_host(p1, p2, f)
        assert C.find_reads_device(x, y, "overmatched=true") == C.find_reads_host(p1, p2, "overmatched=true")


def adam_file(path, reads):
    """ADAMRecord Parquet of compare.Read records (the columns compare projects)"""
    import pyarrow as pa
    import pyarrow.parquet as pq

    def qual(r):
        return None if r.quals is None else "".join(chr((q + 33) & 0xFF) for q in r.quals)

    t = pa.table({
        "readName": pa.array([None if r.name is None else r.name.decode("latin-1") for r in reads], pa.string()),
        "recordGroupId": pa.array([r.rg for r in reads], pa.int32()),
        "readMapped": pa.array([r.mapped for r in reads], pa.bool_()),
        "primaryAlignment": pa.array([r.primary for r in reads], pa.bool_()),
        "readPaired": pa.array([r.paired for r in reads], pa.bool_()),
        "firstOfPair": pa.array([r.first for r in reads], pa.bool_()),
        "duplicateRead": pa.array([r.dup for r in reads], pa.bool_()),
        "referenceId": pa.array([r.reference_id for r in reads], pa.int32()),
        "referenceName": pa.array([r.reference_name for r in reads], pa.string()),
        "start": pa.array([r.start for r in reads], pa.int64()),
        "mapq": pa.array([r.mapq for r in reads], pa.int32()),
        "qual": pa.array([qual(r) for r in reads], pa.string()),
    })
    pq.write_table(t, path, row_group_size=7)
    return path


def R(name, i, **kw):
    d = dict(name=name, index=i, rg=0, mapped=True, primary=True, paired=False, first=False, dup=False,
             reference_id=0, reference_name="c", start=10 + i, mapq=30, quals=[40, 41, 42])
    d.update(kw)
    return C.Read(**d)


def test_adam_nulls(tmp_path):
    # what only Parquet can hold: a null boolean reads as false, a null readName is one name of its
    # own (distinct from ""), mapq may be any int32, a null qual unboxes under baseqs only
    r1 = [R(b"a", 0), R(None, 1), R(b"", 2), R(None, 3, rg=1), R(b"b", 4, mapped=None), R(b"c", 5, paired=True, first=None),
          R(b"d", 6, primary=None), R(b"e", 7, mapq=-7), R(b"f", 8, dup=None), R(b"g", 9, rg=None)] + \
         [R(b"n%d" % i, 10 + i) for i in range(20)]
    r2 = [R(b"a", 0, start=15), R(None, 1, quals=[40, 0, -95]), R(b"", 2), R(b"b", 3), R(b"c", 4, paired=True, first=False),
          R(b"d", 5, primary=False), R(b"e", 6, mapq=1 << 30), R(b"f", 7, dup=True), R(b"g", 8, rg=None)] + \
         [R(b"n%d" % i, 9 + i, quals=[40, 41]) for i in range(20)]
    # the host records as Parquet reads them back: a null boolean is false
    def host(reads):
        return [C.Read(**{k: (False if v is None and k in ("mapped", "primary", "paired", "first", "dup") else v)
                          for k, v in vars(r).items()}) for r in reads]
    p1, p2 = adam_file(str(tmp_path / "1.adam"), r1), adam_file(str(tmp_path / "2.adam"), r2)
    want = C.compare_reads(host(r1), host(r2), ALL)
    same(C.compare_device(p1, p2, ALL), want)
    assert (want.total1, want.unique1) == (30, 0) and want.histograms["mapqs"][(-7, 1 << 30)] == 1
    assert want.histograms["overmatched"][True] >= 25 and (42, -95) in want.histograms["baseqs"]
    name, rows = C.find_reads_device(p1, p2, "baseqs=(42,-95)")
    assert rows == [("null", "c:11", "c:11"), ("null", "c:13", "c:11")]  # both null-named buckets of input 1 join it
    # a null qual: NULL_FIELD under baseqs only, naming the side and the read
    r2[12] = R(b"n3", 12, quals=None)
    r1[20] = R(b"n10", 20, quals=None)
    r1[25] = R(b"n15", 25, quals=None)
    p1, p2 = adam_file(str(tmp_path / "3.adam"), r1), adam_file(str(tmp_path / "4.adam"), r2)
    for comps in (["baseqs"], ALL):
        with pytest.raises(C.CompareNullField) as e:
            C.compare_device(p1, p2, comps)
        with pytest.raises(C.CompareNullField) as h:
            C.compare_reads(host(r1), host(r2), comps)
        assert (e.value.comparison, e.value.side, e.value.read) == (h.value.comparison, h.value.side, h.value.read) \
            == ("baseqs", 1, 20)
    others = ["overmatched", "dupemismatch", "positions", "mapqs"]
    same(C.compare_device(p1, p2, others), C.compare_reads(host(r1), host(r2), others))
    # a null start / mapq in Parquet
    r1[14] = R(b"n4", 14, start=None)
    r2[15] = R(b"n6", 15, mapq=None)
    p1, p2 = adam_file(str(tmp_path / "5.adam"), r1), adam_file(str(tmp_path / "6.adam"), r2)
    for comps, exp in ((["positions"], ("positions", 1, 14)), (["mapqs"], ("mapqs", 2, 15))):
        with pytest.raises(C.CompareNullField) as e:
            C.compare_device(p1, p2, comps)
        assert (e.value.comparison, e.value.side, e.value.read) == exp


def _hashes(sam):
    keys, names = set(), set()
    for line in sam.split(b"\n"):
        f = line.split(b"\t")
        if len(f) > 10 and not line.startswith(b"@"):
            rg = [t[5:] for t in f[11:] if t.startswith(b"RG:Z:")]
            rg = {b"g": 0, b"h": 1}.get(rg[0]) if rg else None
            keys.add((rg, f[0]))
            names.add(f[0])
    return keys, names


def test_collisions(tmp_path):
    p1, p2 = write_pair(tmp_path, gen_pair(31, 300))
    host = C.compare_host(p1, p2, ALL)
    # 8 bits, about 300 names: the bucketing meets a collision and SAM text falls back to the host path
    dev = C.compare_device(p1, p2, ALL, _hash_bits=8)
    same(dev, host)
    assert dev.stats.get("fallback") == "host"
    # a mask that leaves each input's buckets distinct while different names of the two inputs collide:
    # the join compares bytes, no fallback
    bits = None
    for seed in range(500, 540):
        sams = gen_pair(seed, 150)
        sides = []
        for s in sams:
            keys, names = _hashes(s)
            sides.append(([bucket_hash(g, n) for g, n in keys], {n: fnv1a(n) for n in names}))
        for b in range(10, 24):
            mask = (1 << b) - 1
            if any(len({h & mask for h in ks}) != len(ks) for ks, _ in sides):
                continue
            there = {}
            for n, h in sides[1][1].items():
                there.setdefault(h & mask, set()).add(n)
            if any(there.get(h & mask, {n}) != {n} for n, h in sides[0][1].items()):
                bits = b
                break
        if bits:
            break
    assert bits, "no seed and mask separate the buckets of each input while names of the two collide"
    p1, p2 = write_pair(tmp_path, sams, "j")
    host = C.compare_host(p1, p2, ALL)
    dev = C.compare_device(p1, p2, ALL, _hash_bits=bits)
    same(dev, host)
    assert "fallback" not in dev.stats
    assert C.find_reads_device(p1, p2, "overmatched=false", _hash_bits=bits) == C.find_reads_host(
        p1, p2, "overmatched=false")
    # a BAM or ADAM input has no host path: the documented status
    from adam_amd.transform import transform
    q1, q2 = write_pair(tmp_path, gen_pair(32, 300, wide=False), "q")
    b1, a2 = str(tmp_path / "1.bam"), str(tmp_path / "2.adam")
    transform(q1, b1)
    transform(q2, a2)
    for x, y in ((b1, q2), (q1, a2), (b1, a2)):
        with pytest.raises(_capi.BQSRError) as e:
            C.compare_device(x, y, ALL, _hash_bits=8)
        assert e.value.status == _capi.UNSUPPORTED and "share a 8-bit hash" in str(e.value)


def _null(p1, p2, comparisons):
    got = []
    for f in (C.compare_host, C.compare_device):
        with pytest.raises(C.CompareNullField) as e:
            f(p1, p2, comparisons)
        assert e.value.status == _capi.NULL_FIELD
        got.append((e.value.comparison, e.value.side, e.value.read))
    assert got[0] == got[1]
    return got[1]


def test_null_fields(tmp_path):
    body = b"".join(rec(b"r%d" % i, 16, b"IIII") for i in range(70))
    # mapq: MAPQ 255 on reads 71 and 73 of input 1 and on read 66 of input 2 -> side 1, read 71
    f1 = body + rec(b"x", 16, b"II") + rec(b"y", 16, b"II", mapq=255) + rec(b"z", 16, b"II") + rec(b"w", 16, b"II", mapq=255)
    f2 = b"".join(rec(b"r%d" % i, 16, b"IIII") for i in range(66)) + rec(b"x", 16, b"II", mapq=255) + \
        rec(b"y", 16, b"II") + rec(b"z", 16, b"II") + rec(b"w", 16, b"II")
    p1, p2 = write_pair(tmp_path, (HDR + f1, HDR + f2))
    assert _null(p1, p2, ["mapqs"]) == ("mapqs", 1, 71)
    assert _null(p1, p2, ALL) == ("mapqs", 1, 71)
    # only input 2 holds one
    p1b, p2b = write_pair(tmp_path, (HDR + body + rec(b"x", 16, b"II"), HDR + f2), "b")
    assert _null(p1b, p2b, ["mapqs"]) == ("mapqs", 2, 66)
    # an unselected comparison never fails the job
    r = C.compare_device(p1, p2, ["overmatched", "dupemismatch", "positions", "baseqs"])
    same(r, C.compare_host(p1, p2, ["overmatched", "dupemismatch", "positions", "baseqs"]))
    # start: RNAME '*' on both sides (two null referenceIds compare equal); RNAME '*' makes mapq null too,
    # and positions comes first
    g1 = body + rec(b"s", 16, b"II", ref=b"*") + rec(b"t", 16, b"II", pos=0)
    g2 = rec(b"t", 16, b"II") + body + rec(b"s", 16, b"II", ref=b"*")
    p1, p2 = write_pair(tmp_path, (HDR + g1, HDR + g2), "s")
    assert _null(p1, p2, ["positions"]) == ("positions", 1, 70)
    assert _null(p1, p2, ALL) == ("positions", 1, 70)
    assert _null(p1, p2, ["mapqs", "baseqs"]) == ("mapqs", 1, 70)
    same(C.compare_device(p1, p2, ["baseqs", "dupemismatch"]), C.compare_host(p1, p2, ["baseqs", "dupemismatch"]))
    # a null start on one side only, referenceIds differ: -1, no failure
    p1, p2 = write_pair(tmp_path, (HDR + rec(b"a", 16, b"II", ref=b"*"), HDR + rec(b"a", 16, b"II")), "d")
    same(C.compare_device(p1, p2, ["positions"]), C.compare_host(p1, p2, ["positions"]))


def test_findreads(big):
    p1, p2, _ = big
    with pytest.raises(ValueError) as e:
        C.find_reads_device(p1, p2, "positions!=0")
    assert str(e.value) == '"0" isn\'t a legal filter value for positions'
    host = {}
    for f in ("positions>0", "dupemismatch=(1,0)", "overmatched=false", "baseqs!=(40,40);mapqs=(60,60)",
              "positions<0;overmatched=false", "positions=0;baseqs=(5,5)", "mapqs!=(60,60);dupemismatch!=(0,0)",
              "overmatched=true;baseqs=(-95,-95)"):
        name, rows = C.find_reads_device(p1, p2, f)
        hname, host[f] = C.find_reads_host(p1, p2, f)
        assert name == hname and rows == host[f], f
    assert len(host["positions>0"]) > 50 and len(host["dupemismatch=(1,0)"]) > 5 and len(host["overmatched=false"]) > 5


def test_findreads_cli(tmp_path, capsys):
    from adam_amd import findreads
    p1, p2 = write_pair(tmp_path, gen_pair(41, 100))
    assert findreads.main([p1, p2, "positions>0"]) == 0
    assert capsys.readouterr().out == C.find_reads_text(*C.find_reads_host(p1, p2, "positions>0"))
    out = tmp_path / "rows.txt"
    assert findreads.main([p1, p2, "overmatched=false", "-file", str(out)]) == 0
    assert out.read_bytes().decode("latin-1") == C.find_reads_text(*C.find_reads_host(p1, p2, "overmatched=false"))
