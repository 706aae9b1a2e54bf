"""Test infrastructure: a per-record Python restatement of adam2sam's line
rules (include/adam_sam.h at bqsr_arrow_sam_lines) -- a dict of ADAMRecord
fields (adam.avdl names, None = null, as tests/_adam_ref.convert_sam makes
them) gives one SAM line -- and of the header synthesis (parquet.sam_header)
from a list of such dicts.  Also the generator of canonical SAM the round
trips use, and the dicts as a pyarrow table.  Not used by the product.

The line is the inverse of SAMRecordConverter.convert
(adam-core/.../converters/SAMRecordConverter.scala:26-144); where the
converter loses information the header states the choice, restated here:
FLAG 0 for eleven false booleans, MAPQ 255 / 0 for a null mapq with / without
a referenceName, TLEN 0, the attributes reversed and MD last.
"""
from __future__ import annotations

import re
from datetime import datetime, timedelta, timezone
from typing import Dict, List, Optional, Sequence

import numpy as np

BOOLS = ("readPaired", "properPair", "readMapped", "mateMapped", "readNegativeStrand", "mateNegativeStrand",
         "firstOfPair", "secondOfPair", "primaryAlignment", "failedVendorQualityChecks", "duplicateRead")
STRINGS = ("readName", "cigar", "sequence", "qual", "mismatchingPositions")
RG_FIELDS = (("CN", "recordGroupSequencingCenter"), ("DS", "recordGroupDescription"),
             ("DT", "recordGroupRunDateEpoch"), ("FO", "recordGroupFlowOrder"), ("KS", "recordGroupKeySequence"),
             ("LB", "recordGroupLibrary"), ("PI", "recordGroupPredictedMedianInsertSize"),
             ("PL", "recordGroupPlatform"), ("PU", "recordGroupPlatformUnit"), ("SM", "recordGroupSample"))
ATTRIBUTE = re.compile(r"[A-Za-z][A-Za-z0-9]:[AifZHB]:[^\t]*\Z", re.S)
MAX_START = 2 ** 31 - 2


class Malformed(ValueError):
    """the record is refused as malformed (SAM_PARSE)"""


class Unrepresentable(ValueError):
    """the record is refused as one SAM cannot hold (UNSUPPORTED)"""


def flag_of(rec: dict) -> int:
    b = {k: bool(rec.get(k)) for k in BOOLS}  # a null boolean reads as false
    if not any(b.values()):
        return 0
    return (0x1 * b["readPaired"] | 0x2 * b["properPair"] | 0x4 * (not b["readMapped"])
            | 0x8 * (b["readPaired"] and not b["mateMapped"]) | 0x10 * b["readNegativeStrand"]
            | 0x20 * b["mateNegativeStrand"] | 0x40 * b["firstOfPair"] | 0x80 * b["secondOfPair"]
            | 0x100 * (not b["primaryAlignment"]) | 0x200 * b["failedVendorQualityChecks"]
            | 0x400 * b["duplicateRead"])


def line(rec: dict) -> str:
    """One record's SAM line, without the newline.  Strings are text whose
    chars are the column's bytes (Latin-1)."""
    malformed = unrepresentable = False
    for k in STRINGS:
        if re.search(r"[\t\n\r]", rec.get(k) or ""):
            unrepresentable = True
    attrs = rec.get("attributes") or ""
    if re.search(r"[\n\r]", attrs):
        unrepresentable = True
    fields = attrs.split("\t") if attrs else []
    if not all(ATTRIBUTE.match(f) for f in fields):
        malformed = True
    for k in ("start", "mateAlignmentStart"):
        if rec.get(k) is not None and not 0 <= rec[k] <= MAX_START:
            unrepresentable = True
    if rec.get("mapq") is not None and not 0 <= rec["mapq"] <= 255:
        unrepresentable = True
    if malformed:
        raise Malformed(rec)
    if unrepresentable:
        raise Unrepresentable(rec)
    star = lambda v: v if v else "*"  # noqa: E731
    pos = lambda v: 0 if v is None else v + 1  # noqa: E731
    rname, mate = rec.get("referenceName"), rec.get("mateReference")
    mapq = rec.get("mapq")
    if mapq is None:
        mapq = 255 if rname is not None else 0
    out = [star(rec.get("readName")), str(flag_of(rec)), "*" if rname is None else rname, str(pos(rec.get("start"))),
           str(mapq), star(rec.get("cigar")), "*" if mate is None else "=" if mate == rname else mate,
           str(pos(rec.get("mateAlignmentStart"))), "0", star(rec.get("sequence")), star(rec.get("qual"))]
    out += fields[::-1]
    if rec.get("mismatchingPositions") is not None:
        out.append("MD:Z:" + rec["mismatchingPositions"])
    return "\t".join(out)


def lines(recs: Sequence[dict]) -> bytes:
    return "".join(line(r) + "\n" for r in recs).encode("latin-1")


def epoch_ms_iso8601(ms: int) -> str:
    t = datetime(1970, 1, 1, tzinfo=timezone.utc) + timedelta(milliseconds=ms)
    return t.strftime("%Y-%m-%dT%H:%M:%S") + (".%03d" % (ms % 1000) if ms % 1000 else "") + "Z"


def header(recs: Sequence[dict]) -> bytes:
    """The header parquet.sam_header synthesises: @SQ lines by ascending id
    from the records' own and their mates' (id, name, length, URL), @RG lines
    sorted by ID; ValueError on the conflicts it refuses."""
    sq = set()
    for r in recs:
        if r.get("referenceName") is not None:
            sq.add((r.get("referenceId"), r["referenceName"], r.get("referenceLength"), r.get("referenceUrl")))
        if r.get("mateReference") is not None:
            sq.add((r.get("mateReferenceId"), r["mateReference"], r.get("mateReferenceLength"),
                    r.get("mateReferenceUrl")))
    names = [q[1] for q in sq]
    ids = [q[0] for q in sq if q[0] is not None]
    if len(set(names)) != len(names) or len(set(ids)) != len(ids):
        raise ValueError("conflicting contigs: %r" % sorted(sq, key=repr))
    out = []
    for rid, name, length, url in sorted(sq, key=lambda q: (q[0] is None, q[0] or 0, q[1])):
        out.append("\t".join(["@SQ", "SN:" + name] + (["LN:%d" % length] if length is not None else [])
                             + (["UR:" + url] if url is not None else [])))
    rg: Dict[str, tuple] = {}
    for r in recs:
        if r.get("recordGroupName") is not None:
            v = tuple(r.get(c) for _, c in RG_FIELDS)
            if rg.setdefault(r["recordGroupName"], v) != v:
                raise ValueError("conflicting read group %r" % r["recordGroupName"])
    for name in sorted(rg):
        f = ["@RG", "ID:" + name]
        for (tag, _c), v in zip(RG_FIELDS, rg[name]):
            if v is not None:
                f.append("%s:%s" % (tag, epoch_ms_iso8601(v) if tag == "DT" else v))
        out.append("\t".join(f))
    return "".join(l + "\n" for l in out).encode("latin-1")


# ---- the records as a table ----

def table(recs: Sequence[dict], cuts: Sequence[int] = ()):
    """The dicts as a pyarrow table of ADAMRecord columns (adam_save.schema),
    strings as Latin-1 text; cut into record batches at the rows `cuts`."""
    import pyarrow as pa

    from adam_amd.adam_save import schema
    sch = schema()
    cols = {f.name: pa.array([r.get(f.name) for r in recs], f.type) for f in sch}
    t = pa.table(cols, schema=sch)
    if not cuts:
        return t
    edges = [0] + list(cuts) + [len(recs)]
    # (slices of one table: the arrays of every batch but the first carry an offset that is no multiple of 8)
    return pa.Table.from_batches([b for a, z in zip(edges, edges[1:]) for b in t.slice(a, z - a).to_batches()], sch)


# ---- canonical SAM: text the round trip reproduces byte for byte ----

HEAD = (b"@HD\tVN:1.4\tSO:unsorted\n@SQ\tSN:chr1\tLN:250000000\n@SQ\tSN:chr2\tLN:200000000\tUR:file:/ref.fa\n"
        b"@SQ\tSN:chrUn\tLN:5000\n@RG\tID:rgB\tSM:s2\tLB:lib2\tPL:illumina\n"
        b"@RG\tID:rgA\tSM:s1\tLB:lib1\tCN:here\tDT:2013-02-03T04:05:06Z\tPI:300\n@CO\tnot carried by ADAMRecord\n")
CONTIGS = ("chr1", "chr2")  # (chrUn stays unused: only -header_from brings it back)


def canonical_sam(n: int, seed: int = 1, lens: Sequence[int] = (0, 1, 63, 64, 65, 300)) -> bytes:
    """n records of canonical SAM under HEAD: TLEN 0, "=" for an equal RNEXT,
    pair bits only with 0x1, no FLAG 0x104, MAPQ != 255 on placed reads and 0
    on unplaced ones, canonical CIGAR, tags of types A / i / f / Z in
    htsjdk's order (second char, then first) with MD last."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ln = int(lens[i % len(lens)]) if i < 2 * len(lens) else int(rng.integers(20, 120))
        placed = rng.random() < 0.85
        paired = rng.random() < 0.6
        flag = 0
        if paired:
            flag |= 0x1 | int(rng.choice([0, 0x2])) | int(rng.choice([0, 0x8])) | int(rng.choice([0, 0x20]))
            flag |= int(rng.choice([0x40, 0x80]))
        flag |= int(rng.choice([0, 0x10])) | int(rng.choice([0, 0x200])) | int(rng.choice([0, 0x400]))
        if not placed or rng.random() < 0.1:
            flag |= 0x4
        if rng.random() < 0.1:
            flag |= 0x100
        if flag == 0x104:
            flag = 0x4
        rname = str(rng.choice(CONTIGS)) if placed else "*"
        pos = int(rng.integers(1, 1_000_000)) if placed else 0
        mapq = int(rng.integers(0, 255)) if placed else 0
        seq = "".join(rng.choice(list("ACGTN"), ln)) if ln else "*"
        qual = "".join(chr(int(q)) for q in rng.integers(33, 74, ln)) if ln and rng.random() < 0.9 else "*"
        cigar = "%dM" % ln if ln and placed and not flag & 0x4 else "*"
        if paired and rng.random() < 0.8:
            rnext = rname if placed and rng.random() < 0.7 else str(rng.choice(CONTIGS))
            pnext = int(rng.integers(1, 1_000_000))
        else:
            rnext, pnext = "*", 0
        tags = {}
        if rng.random() < 0.8:
            tags["RG"] = "Z:" + str(rng.choice(["rgA", "rgB"]))
        if rng.random() < 0.5:
            tags["NM"] = "i:%d" % rng.integers(-3, 50)
        if rng.random() < 0.3:
            tags["XT"] = "A:" + str(rng.choice(list("URM")))
        if rng.random() < 0.3:
            tags["XF"] = "f:" + str(rng.choice(["1.5", "0.25", "-3.0", "100.0"]))
        if rng.random() < 0.2:
            tags["X0"] = "Z:"
        if i % 7 == 3:
            tags["XL"] = "Z:" + "x" * [63, 64, 65, 300][i % 4]
        if placed and rng.random() < 0.7:
            tags["MD"] = "Z:%d" % ln
        order = sorted((t for t in tags if t != "MD"), key=lambda t: (t[1], t[0])) + (["MD"] if "MD" in tags else [])
        f = ["r%d" % i, str(flag), rname, str(pos), str(mapq), cigar, "=" if rnext == rname != "*" else rnext,
             str(pnext), "0", seq, qual] + ["%s:%s" % (t, tags[t]) for t in order]
        out.append("\t".join(f))
    return HEAD + "".join(l + "\n" for l in out).encode()


def body(text: bytes) -> bytes:
    return b"".join(l + b"\n" for l in text.split(b"\n") if l and not l.startswith(b"@"))


def head(text: bytes) -> bytes:
    return b"".join(l + b"\n" for l in text.split(b"\n") if l.startswith(b"@"))


def run_date(v: str) -> Optional[int]:
    from adam_amd.adam_save import _iso8601_epoch_ms
    return _iso8601_epoch_ms(v)
