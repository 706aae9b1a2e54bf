"""Generated reads for the pileup tests: random CIGARs over all nine operators
with an MD tag consistent with them (the way the reference reads it: the MD
offset is referencePos - start, so N, = and X spans count as matches), and
the helpers that compare a device table with the restatement's rows."""
import functools
import random

import _adam_ref
import _pileup_ref as PR

HEADER = (b"@HD\tVN:1.4\n"
          b"@SQ\tSN:c1\tLN:100000000\n@SQ\tSN:c2\tLN:50000000\tUR:file:/x\n@SQ\tSN:c3\tLN:7\n"
          b"@RG\tID:g2\tSM:s2\tLB:lib2\tPL:illumina\tCN:center\tDS:a description\tPU:unit\tPI:300\tFO:ACGT\tKS:TG\n"
          b"@RG\tID:g0\tSM:s0\tLB:lib0\tDT:2013-11-07T10:30:00Z\n"
          b"@RG\tID:g1\tSM:s1\n")
IUPAC = "UKMRYSWBVHDXN"
MD_LETTERS = "AGCTNUKMRSWBVHDXY"


def run_date(v):
    from adam_amd.adam_save import _iso8601_epoch_ms
    return _iso8601_epoch_ms(v)


def _bases(rnd, n, iupac=IUPAC):
    return "".join(rnd.choice(iupac) if rnd.randrange(12) == 0 else rnd.choice("ACGT") for _ in range(n))


def _quals(rnd, n, wide=True):
    out = []
    for _ in range(n):
        k = rnd.randrange(16)
        out.append(126 if k == 0 else rnd.randrange(161, 256) if k == 1 and wide else rnd.randrange(33, 127))
    return bytes(out)


def md_of(rnd, kinds):
    """MD text of a per-reference-offset list: None (match), ('X', base) a
    mismatch, ('D', base) a deleted base"""
    out, run, prev = [], 0, None
    for k in kinds:
        if k is None:
            run += 1
            prev = None
            continue
        letter = k[1].lower() if rnd.randrange(3) == 0 else k[1]
        if prev == k[0] and run == 0 and (k[0] == "D" or rnd.randrange(2)):
            out.append(letter)  # the group goes on
        else:
            out.append(str(run))
            out.append(("^" if k[0] == "D" else "") + letter)
        run, prev = 0, k[0]
    out.append(str(run))
    return "".join(out)


def read_fields(rnd, read_len, ops="MIDNSHP=X", empty=None, iupac=IUPAC, wide=True):
    """(cigar, sequence, qual bytes, md or None) of one read of about read_len
    bases; empty: 'nomd' / 'star' / 'skips' for a read without pileups"""
    if empty == "star":
        return "*", _bases(rnd, max(1, read_len), iupac), _quals(rnd, max(1, read_len), wide), "0" if rnd.randrange(2) else ""
    els = []
    if empty == "skips":
        for _ in range(rnd.randrange(1, 5)):
            els.append((rnd.randrange(1, 9), rnd.choice("NHP=X")))
    else:
        left = read_len
        if "H" in ops and rnd.randrange(6) == 0:
            els.append((rnd.randrange(1, 5), "H"))
        if "S" in ops and left > 2 and rnd.randrange(4) == 0:
            k = rnd.randrange(1, min(6, left))
            els.append((k, "S"))
            left -= k
        tail = []
        if "S" in ops and left > 2 and rnd.randrange(4) == 0:
            k = rnd.randrange(1, min(6, left))
            tail.append((k, "S"))
            left -= k
        if "H" in ops and rnd.randrange(6) == 0:
            tail.append((rnd.randrange(1, 5), "H"))
        body = [o for o in ops if o in "MIDNP=X"]
        while left > 0:
            op = "M" if rnd.randrange(3) else rnd.choice(body)
            k = rnd.randrange(1, 8) if op != "M" else rnd.randrange(1, max(2, left + 1))
            if op in "MI=X":
                k = min(k, left)
                left -= k
            els.append((k, op))
        if els and els[-1][1] == "D":  # (a trailing D throws: its quality is the next read base's)
            els.append((1, "M"))
            left -= 1
        els += tail
    n_read = sum(k for k, op in els if op in "MIS=X")
    seq = _bases(rnd, n_read, iupac) if n_read else "*"
    qual = _quals(rnd, n_read, wide) if n_read else b"*"
    kinds = []
    for k, op in els:
        if op == "M":
            kinds += [("X", rnd.choice(MD_LETTERS)) if rnd.randrange(8) == 0 else None for _ in range(k)]
        elif op == "D":
            kinds += [("D", rnd.choice(MD_LETTERS)) for _ in range(k)]
        elif op in "N=X":
            kinds += [None] * k
    md = None if empty == "nomd" else md_of(rnd, kinds)
    return "".join("%d%s" % e for e in els), seq, qual, md


def sam_line(i, rnd, fields, flag=None, rname=None, mapq=None):
    cigar, seq, qual, md = fields
    if flag is None:
        flag = rnd.choice((16, 1 | 64, 1 | 128 | 16, 256, 512 | 16, 1024, 1 | 2 | 32, 2048))
    rname = rnd.choice(("c1", "c1", "c2", "c3")) if rname is None else rname
    mapq = rnd.choice((0, 7, 30, 60, 255)) if mapq is None else mapq
    tags = []
    rg = rnd.choice((None, "g0", "g1", "g2", "gx"))
    if rg:
        tags.append(b"RG:Z:" + rg.encode())
    if md is not None:
        tags.append(b"MD:Z:" + md.encode())
    if rnd.randrange(2):
        tags.append(b"NM:i:%d" % rnd.randrange(5))
    rnd.shuffle(tags)
    return b"\t".join([b"read%d" % i, b"%d" % flag, rname.encode(), b"%d" % (1 + rnd.randrange(90_000_000)),
                       b"%d" % mapq, cigar.encode(), b"*", b"0", b"0", seq.encode(), qual] + tags) + b"\n"


def _rows(rec):
    try:
        return PR.read_to_pileups(rec)
    except PR.PileupThrow:
        return None


def records(specs, seed, bam_safe=False):
    """(lines, dicts, per-read restatement rows): one generated read per spec
    (read_len, empty[, ops]); a read the restatement throws on is generated again;
    bam_safe: only what survives the BAM and ADAM forms of the text --
    bases BAM's 4-bit codes hold (no U, no X) and ASCII quals (the ADAM
    columns copy a SAM line's QUAL bytes as they are, and bytes beyond 0x7F
    are no UTF-8)"""
    iupac = IUPAC.replace("U", "").replace("X", "") if bam_safe else IUPAC
    rnd = random.Random(seed)
    n = len(specs)
    lines, recs, rows = [None] * n, [None] * n, [None] * n
    todo = list(range(n))
    while todo:
        for i in todo:
            read_len, empty, *rest = specs[i]
            ops = rest[0] if rest else "MIDNSHP=X"
            rname = "*" if empty and rnd.randrange(3) == 0 else None
            flag = 0 if empty and rnd.randrange(3) == 0 else None
            lines[i] = sam_line(i, rnd, read_fields(rnd, read_len, ops, empty=empty, iupac=iupac, wide=not bam_safe), flag=flag, rname=rname)
        for i, r in zip(todo, _adam_ref.convert_sam(HEADER + b"".join(lines[i] for i in todo), run_date)):
            recs[i], rows[i] = r, _rows(r)
        todo = [i for i in todo if rows[i] is None]
    return lines, recs, rows


@functools.lru_cache(maxsize=None)
def generated(specs, seed, bam_safe=False):
    """(SAM text, record dicts, per-read restatement rows), computed once"""
    lines, recs, rows = records(specs, seed, bam_safe)
    return HEADER + b"".join(lines), recs, rows


def flat(per_read, a=0, b=None):
    return [row for rows in per_read[a:b] for row in rows]


def expected_table(rows):
    import pyarrow as pa
    from adam_amd.adam_save import pileup_schema
    sch = pileup_schema()
    return pa.table([pa.array([r[f.name] for r in rows], f.type) for f in sch], schema=sch)


def plain(table):
    """the device table with its dictionary columns decoded"""
    import pyarrow as pa
    from adam_amd.adam_save import pileup_schema
    sch = pileup_schema()
    assert table.column_names == sch.names
    return pa.table([table.column(f.name).cast(f.type).combine_chunks() for f in sch], schema=sch)


def assert_rows(table, rows):
    """every column and validity bit of `table` equals the restatement's rows, in order"""
    got, want = plain(table), expected_table(rows)
    assert got.num_rows == want.num_rows, (got.num_rows, want.num_rows)
    for name in want.column_names:
        g, w = got.column(name), want.column(name)
        if not g.equals(w):
            gl, wl = g.to_pylist(), w.to_pylist()
            k = next(i for i in range(len(wl)) if gl[i] != wl[i])
            raise AssertionError("column %s differs at row %d: got %r, want %r (readName %r)" %
                                 (name, k, gl[k], wl[k], rows[k]["readName"]))
