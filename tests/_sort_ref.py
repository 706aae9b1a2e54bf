"""`transform -sort_reads` restated from the Scala, for the tests
(adamSortReadsByReferencePosition, core/rdd/AdamRDDFunctions.scala:63-93;
ReferencePosition, models/ReferencePosition.scala:73-95,155-166).  Not used
by the product.

The reference maps every read to a key and sorts by key: a mapped read's key
is its ReferencePosition; every other read gets (Int.MaxValue - c,
Long.MaxValue), c from an iterator that counts 1 .. 10000 and then wraps to 0
(:70-82).

ReferencePosition(record) (:73-95) is built only for `readMapped` records,
from record.getReferenceId and record.getStart: either being null is a
NullPointerException (the Option check wraps them in Some(...)).  compare
(:155-166): by refId, then by pos.  One partition: the counter is
deserialised once, and sortWith over the partition's array is stable.
"""
from __future__ import annotations

import random
from typing import List, Optional, Sequence, Tuple

INT_MAX = 2 ** 31 - 1
LONG_MAX = 2 ** 63 - 1
WRAP = 10001  # the counter's values: 1 .. 10000, then 0


def sort_keys_ref(read_mapped: Sequence, reference_id: Sequence, start: Sequence) -> List[Tuple[int, int]]:
    """the (Int, Long) key of every read; raises on a mapped read with a null field"""
    keys = []
    n_unmapped = 0
    for i, (m, r, s) in enumerate(zip(read_mapped, reference_id, start)):
        if m:
            if r is None or s is None:
                raise TypeError("read %d: mapped with a null referenceId or start (NullPointerException)" % i)
            keys.append((int(r), int(s)))
        else:
            n_unmapped += 1
            keys.append((INT_MAX - n_unmapped % WRAP, LONG_MAX))
    return keys


def sort_order_ref(read_mapped: Sequence, reference_id: Sequence, start: Sequence) -> List[int]:
    """order[i] = the input index of the read at sorted position i"""
    keys = sort_keys_ref(read_mapped, reference_id, start)
    return sorted(range(len(keys)), key=keys.__getitem__)  # (stable)


def split_sam(text: bytes) -> Tuple[bytes, List[bytes]]:
    """(header bytes, record lines without their line ends); empty lines dropped"""
    pos = 0
    n = len(text)
    while pos < n:
        nl = text.find(b"\n", pos)
        end = n if nl < 0 else nl
        line = text[pos:end].rstrip(b"\r")
        if line and not line.startswith(b"@"):
            break
        pos = n if nl < 0 else nl + 1
    lines = [l.rstrip(b"\r") for l in text[pos:].split(b"\n")]
    return text[:pos], [l for l in lines if l]


def sam_keys(text: bytes):
    """(read_mapped, reference_id, start) of a SAM text's records with
    SAMRecordConverter's semantics (converters/SAMRecordConverter.scala:26-144
    as adam_amd/records.py restates them): flags only when the FLAG word is
    non-zero (Q2), referenceId = the @SQ index of RNAME, start = POS - 1
    unless POS is 0."""
    header, lines = split_sam(text)
    sq: List[str] = []
    for h in header.split(b"\n"):
        f = h.rstrip(b"\r").split(b"\t")
        if f[0] == b"@SQ":
            sq.append(dict(t.split(b":", 1) for t in f[1:] if b":" in t)[b"SN"].decode("latin-1"))
    mapped: List[bool] = []
    ref: List[Optional[int]] = []
    start: List[Optional[int]] = []
    for l in lines:
        f = l.split(b"\t")
        flag, rname, pos = int(f[1]), f[2].decode("latin-1"), f[3]
        mapped.append(flag != 0 and not flag & 0x4)
        known = rname != "*" and rname in sq
        ref.append(sq.index(rname) if known else None)
        start.append(int(pos) - 1 if known and int(pos) != 0 else None)
    return mapped, ref, start


def sorted_sam(text: bytes, order: Optional[Sequence[int]] = None) -> bytes:
    """the header, then the record lines ('\\n'-ended) in the reference's order"""
    header, lines = split_sam(text)
    if order is None:
        order = sort_order_ref(*sam_keys(text))
    return header + b"".join(lines[i] + b"\n" for i in order)


def suite_reads(seed=20131107, n=1000):
    """AdamRDDFunctionsSuite "sorting reads" (:208-228): n reads, each mapped
    with probability 1/2, mapped ones with referenceId < n / 10 and start < 10^6"""
    rnd = random.Random(seed)
    mapped, ref, start = [], [], []
    for _ in range(n):
        m = rnd.random() < 0.5
        mapped.append(m)
        ref.append(rnd.randrange(n // 10) if m else None)
        start.append(rnd.randrange(1000000) if m else None)
    return mapped, ref, start
