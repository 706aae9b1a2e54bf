"""MarkDuplicates on the device through every entry point -- the single parse
(bqsr_sam_mark_duplicates, SAM text and BAM), the partitioned set
(bqsr_dup_set_*) and the Arrow columns (bqsr_arrow_mark_duplicates) -- on the
reads of tests/_markdup_gen.py: the hand-built edge cases side by side and the
dense random sets, compared exactly with oracle/markdup.py (ties by first
appearance on both sides).  Every single-parse comparison also asserts that
the device did the work (SamText.markdup_path() == 0), except past the packed
keys' limits, where the exact reason for the host form is asserted."""
import functools
import os
import subprocess
import sys

import pytest

import markdup as M  # oracle/markdup.py
import _markdup_gen as G
from adam_amd import _capi
from adam_amd import records as R
from adam_amd.sam import DupSet, SamText

pytestmark = pytest.mark.gpu

SETS = ["cases"] + ["random%d" % s for s in G.RANDOM_SEEDS]


@functools.lru_cache(maxsize=None)
def reads_of(which):
    """(reads, the oracle's answer, SAM text) of a SAM-expressible set; shared, never changed."""
    if which == "cases":
        reads, written = G.concat(sam_only=True)
        want = M.mark_duplicates(reads)
        assert want == written
    elif which == "small":
        reads = G.random_reads(300, G.SMALL_SEED)
        want = M.mark_duplicates(reads)
    else:
        reads = G.random_reads(2000, int(which[len("random"):]))
        want = M.mark_duplicates(reads)
    assert sum(want) > 0
    return reads, want, G.sam_text(reads)


@functools.lru_cache(maxsize=None)
def arrow_reads_of(which):
    """As reads_of, with the cases only ADAM records can hold."""
    if which == "cases":
        reads, written = G.concat()
        want = M.mark_duplicates(reads)
        assert want == written
        return reads, want
    return reads_of(which)[:2]


def dup_bits(s):
    return [bool(f & R.F_DUPLICATE) for f in s.batch().flags]


def first_difference(got, want):
    return next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), None)


# ---- the single parse ----

@pytest.mark.parametrize("form", ["sam", "bam"])
@pytest.mark.parametrize("which", SETS)
def test_single_parse(which, form):
    reads, want, text = reads_of(which)
    s = SamText(text) if form == "sam" else SamText(G.bam_bytes(reads), bam=True)
    try:
        assert s.markdup_path() == -1
        n_dup = s.mark_duplicates()
        assert s.markdup_path() == 0
        got = dup_bits(s)
        assert got == want, first_difference(got, want)
        assert n_dup == sum(want)
        source = G.sam_fields(text)
        before = G.sam_fields(s.text())
        if form == "sam":
            assert before == source
        else:  # the BAM's records as SAM lines: the fields MarkDuplicates reads are the text's
            assert [f[:6] + f[9:11] for f in before] == [f[:6] + f[9:11] for f in source]
        s.rewrite()
        after = G.sam_fields(s.text())
        assert len(after) == len(before)
        for r, (a, c) in enumerate(zip(before, after)):
            flag = int(a[1])
            assert int(c[1]) == ((flag | 0x400) if want[r] else (flag & ~0x400)), r
            assert a[0] == c[0] and a[2:] == c[2:], r
    finally:
        s.close()


def test_single_parse_forced_to_the_host_form_says_so():
    """ADAM_BQSR_MARKDUP=host is read once per process: a child process."""
    code = ("import sys; sys.path[:0] = %r\n"
            "import _markdup_gen as G, markdup as M\n"
            "from adam_amd.sam import SamText\n"
            "from adam_amd import records as R\n"
            "reads = G.random_reads(300, G.SMALL_SEED)\n"
            "s = SamText(G.sam_text(reads))\n"
            "n = s.mark_duplicates()\n"
            "got = [bool(f & R.F_DUPLICATE) for f in s.batch().flags]\n"
            "assert got == M.mark_duplicates(reads) and n == sum(got)\n"
            "print('path', s.markdup_path())\n" % ([os.path.dirname(__file__), os.path.dirname(M.__file__),
                                                  os.path.dirname(os.path.dirname(__file__))],))
    env = dict(os.environ, ADAM_BQSR_MARKDUP="host")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split()[-2:] == ["path", "8"]


# ---- the partitioned set ----

def run_dup_set(head, body, cuts, want):
    """The lines body[a:b] of every cut as one partition, in order: add, finish, apply, compare."""
    parts, d = [], DupSet()
    try:
        for a, b in cuts:
            parts.append(SamText(head + b"".join(l + b"\n" for l in body[a:b])))
            d.add(parts[-1])
        n_dup = d.finish()
        got, total = [], 0
        for i, p in enumerate(parts):
            k = d.apply(i, p)
            bits = dup_bits(p)
            assert k == sum(bits), i
            got += bits
            total += k
        assert got == want, first_difference(got, want)
        assert total == n_dup == sum(want)
    finally:
        d.close()
        for p in parts:
            p.close()


def cuts_between_mates(reads):
    """Partition bounds after every read whose successor shares its name: no two
    neighbouring reads of a bucket stay together."""
    bounds = [0] + [i for i in range(1, len(reads)) if reads[i]["name"] == reads[i - 1]["name"]] + [len(reads)]
    return list(zip(bounds[:-1], bounds[1:]))


@pytest.mark.parametrize("split", ["one", "mates", "empty_middle", "uneven"])
@pytest.mark.parametrize("which", ["cases", "random1"])
def test_dup_set(which, split):
    reads, want, _ = reads_of(which)
    n = len(reads)
    body = G.sam_body(reads)
    if split == "one":
        cuts = [(0, n)]
    elif split == "mates":
        cuts = cuts_between_mates(reads if which == "cases" else reads[:600])
        assert len(cuts) > 40
        cuts += [(cuts[-1][1], n)] if cuts[-1][1] < n else []
    elif split == "empty_middle":
        cuts = [(0, n // 3), (n // 3, n // 3), (n // 3, n)]
    else:
        # one-read partitions at both ends, a bound at the edge of a 256-thread block where there is one
        bounds = sorted({0, 1, 2, n // 2, n - 1, n} | ({257, 258} if n > 600 else {7, 8}))
        cuts = list(zip(bounds[:-1], bounds[1:]))
    run_dup_set(G.header(), body, cuts, want)


def test_dup_set_every_read_its_own_partition():
    reads, want, _ = reads_of("small")
    run_dup_set(G.header(), G.sam_body(reads), [(i, i + 1) for i in range(len(reads))], want)


# ---- the Arrow columns ----

@pytest.mark.parametrize("which,chunks", [(w, 1) for w in SETS] + [("cases", 3), ("random1", 3)])
def test_arrow(which, chunks):
    pa = pytest.importorskip("pyarrow")
    from adam_amd import parquet as P
    reads, want = arrow_reads_of(which)
    t = G.arrow_table(reads)
    if chunks > 1:  # as the row groups of a Parquet file arrive: slices with offsets
        n = t.num_rows
        t = pa.concat_tables([t.slice(0, 7), t.slice(7, n // 2 - 7), t.slice(n // 2)])
        assert t.column("readName").num_chunks == 3
    A = P.ArrowReads(t, markdup=True)
    try:
        n_dup = A.mark_duplicates()
        got = A.flag_column(R.F_DUPLICATE).to_pylist()
    finally:
        A.close()
    assert got == want, first_difference(got, want)
    assert n_dup == sum(want)


@pytest.mark.parametrize("which", ["cases", "random2"])
def test_transform_adam_writes_the_duplicate_column(tmp_path, which):
    pytest.importorskip("pyarrow")
    import pyarrow.parquet as pq
    from adam_amd.transform import transform
    reads, want = arrow_reads_of(which)
    inp, out = str(tmp_path / "in.adam"), str(tmp_path / "out.adam")
    pq.write_table(G.arrow_table(reads), inp)
    st = transform(inp, out, mark_duplicates=True)
    t = pq.read_table(out)
    assert t.column("duplicateRead").to_pylist() == want
    assert st["duplicates"] == sum(want)
    assert t.column("readName").to_pylist() == [r["name"] for r in reads]


# ---- the packed keys' limits: 32767 contigs (indices 0..32766), 4095 distinct LB values ----

def limit_reads(spots):
    """About 40 reads around `spots`, each (contig, the contig of its pairs'
    other mates, read group, library): fragments and pairs that are duplicates
    at each spot, at positions the other spots use as well."""
    reads = []
    for k, (ref, far, rg, lib) in enumerate(spots):
        kw = dict(rg=rg, library=lib)
        reads += [G.rd("f%d.%d" % (k, i), ref, 100, phred=p, **kw) for i, p in enumerate((20, 30, 10))]
        reads += [G.rd("r%d.%d" % (k, i), ref, 700, neg=True, phred=p, **kw) for i, p in enumerate((10, 20))]
        for name, phred in (("p", 20), ("q", 30), ("s", 30)):
            a, b = G.mates("%s%d" % (name, k), (far, 300), (ref, 900), phred=phred, **kw)
            reads += [b, a] if name == "q" else [a, b]  # in either order
        reads += [G.rd("x%d" % k, far, 100, neg=True, **kw)]
    return reads


def limit_text(reads, contigs, rg_ids=G.RG_IDS, rg_lib=G.RG_LIB, rg_order=G.RG_HEADER_ORDER):
    head = G.header(contigs, rg_ids, rg_lib, rg_order)
    body = G.sam_body(reads, contigs, rg_ids, rg_lib)
    return head, body


def check_within_limit(head, body, want):
    text = head + b"".join(l + b"\n" for l in body)
    s = SamText(text)
    try:
        n_dup = s.mark_duplicates()
        assert s.markdup_path() == 0
        got = dup_bits(s)
        assert got == want, first_difference(got, want)
        assert n_dup == sum(want)
    finally:
        s.close()
    run_dup_set(head, body, [(0, len(body) // 2), (len(body) // 2, len(body))], want)


def check_past_limit(head, body, want, reason):
    text = head + b"".join(l + b"\n" for l in body)
    s = SamText(text)
    try:
        n_dup = s.mark_duplicates()
        assert s.markdup_path() == reason
        got = dup_bits(s)
        assert got == want, first_difference(got, want)
        assert n_dup == sum(want)
    finally:
        s.close()
    p, d = SamText(text), DupSet()
    try:
        d.add(p)
        with pytest.raises(_capi.BQSRError) as e:
            d.finish()
        assert e.value.status == _capi.UNSUPPORTED
        with pytest.raises(_capi.BQSRError):  # not finished: nothing to apply
            d.apply(0, p)
        assert not any(dup_bits(p))
    finally:
        d.close()
        p.close()


@pytest.mark.parametrize("n_sq,reason", [(32767, 0), (32768, 2)])
def test_contig_limit(n_sq, reason):
    contigs = ["c%05d" % i for i in range(n_sq)]
    last = n_sq - 1
    reads = limit_reads([(0, last, 0, G.RG_LIB[0]), (1, 1, 0, G.RG_LIB[0]), (last, 0, 0, G.RG_LIB[0])])
    reads += [G.rd("y%d" % i, last - 1, 100, phred=p) for i, p in enumerate((30, 20))]  # the contig before the last
    assert 35 <= len(reads) <= 45 and {r["ref"] for r in reads} == {0, 1, last - 1, last}
    want = M.mark_duplicates(reads)
    assert 10 < sum(want) < len(reads)
    head, body = limit_text(reads, contigs)
    assert head.count(b"@SQ\t") == n_sq
    if reason == 0:
        check_within_limit(head, body, want)
    else:
        check_past_limit(head, body, want, reason)


@pytest.mark.parametrize("n_lb,reason", [(4095, 0), (4096, 4)])
def test_library_limit(n_lb, reason):
    # read group i (IDs sorted) names the LB of rank n_lb - i: the last rank belongs to read group 0
    rg_ids = ["g%04d" % i for i in range(n_lb)]
    rg_lib = {i: "L%04d" % (n_lb - 1 - i) for i in range(n_lb)}
    reads = limit_reads([(0, 1, g, rg_lib[g]) for g in (n_lb - 1, n_lb // 2, 0)])  # the first, a middle, the last rank
    reads += [G.rd("none%d" % i, 0, 100, rg=None, phred=p) for i, p in enumerate((10, 20))]  # no library: rank 0
    assert 35 <= len(reads) <= 45
    want = M.mark_duplicates(reads)
    assert 10 < sum(want) < len(reads)
    order = list(range(1, n_lb, 2)) + list(range(0, n_lb, 2))
    head, body = limit_text(reads, G.CONTIGS, rg_ids, rg_lib, order)
    assert head.count(b"\tLB:") == n_lb
    if reason == 0:
        check_within_limit(head, body, want)
    else:
        check_past_limit(head, body, want, reason)
