"""`adam mpileup` restated in plain Python: the yardstick of the mpileup tests.

MpileupCommand.run (adam-cli/.../cli/MpileupCommand.scala:37-82) over
PileupTraversable (adam-core/.../util/PileupTraversable.scala:83-281:
readToPileups :104-192, foreach :194-280 with flushPileups :203-241), MdTag
(util/MdTag.scala:38-98, 247-269) and LocusPredicate
(predicates/LocusPredicate.scala), written from the Scala, statement by
statement, over the ADAMRecord dicts ``_adam_ref.convert_sam`` returns (or
dicts built by hand: a missing key is a null field).  Nothing here knows how
the device does it.

Every Scala exception class is a class here; ``.status`` is the name the C ABI
gives it and ``.read`` the index of the read, in the input, it was thrown for.
Two of them are this project's declarations where the reference is loose
(adam_amd/mpileup.py): :class:`Unsorted` is the reference's "sorted" assert
(:260) made strict -- any decrease of start inside a segment, not only one
below the segment's first start -- and :class:`ReferenceConflict` is the
assert of :230.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional

import _pileup_ref as PR

# PileupTraversable.scala:32-34
BASES = ("A", "C", "T", "G", "N")


class MpileupThrow(Exception):
    status = ""

    def __init__(self, what: str = "", read: int = -1):
        super().__init__("%s: %s" % (self.status, what))
        self.what = what
        self.read = read


class NullPointerException(MpileupThrow):
    status = "NULL_FIELD"


class MdTagRejects(MpileupThrow):  # MdTag.apply's IllegalArgumentException / NumberFormatException
    status = "MD_PARSE"


class NoSuchElementException(MpileupThrow):  # Base.withName
    status = "PILEUP"


class IllegalArgumentException(MpileupThrow):  # :150, :170
    status = "PILEUP"


class StringIndexOutOfBoundsException(MpileupThrow):  # subSequence(pos, pos + 1)
    status = "PILEUP"


class Unsorted(MpileupThrow):  # the assert of :260, any decrease (declared)
    status = "UNSORTED"


class ReferenceConflict(MpileupThrow):  # the assert of :230
    status = "REFERENCE_CONFLICT"

    def __init__(self, reference_name: str, position: int):
        super().__init__("%s %d" % (reference_name, position))
        self.reference_name = reference_name
        self.position = position


def base_with_name(s: str) -> str:
    """Base.withName: the five-value enum of :32-34"""
    if s not in BASES:
        raise NoSuchElementException("None.get: no Base " + repr(s))
    return s


def read_to_pileups(rec: dict) -> List[dict]:
    """readToPileups(record), :104-192: single-event Pileups, in the order of
    the returned list (built by prepending: reverse walk order)."""
    g = rec.get
    if g("cigar") is None or g("mismatchingPositions") is None:  # :105
        return []

    def need(key):  # a null dereferenced or unboxed
        v = g(key)
        if v is None:
            raise NullPointerException(key)
        return v

    def base_from_sequence(pos):  # :111-114
        s = need("sequence")
        if pos + 1 > len(s):
            raise StringIndexOutOfBoundsException("sequence index %d" % pos)
        return base_with_name(s[pos])

    reference_pos = g("start")  # :116 (boxed)
    read_pos = 0
    cigar = PR.decode_cigar(g("cigar"))  # :120
    if reference_pos is None:  # :121 MdTag(md, referencePos) unboxes
        raise NullPointerException("start")
    try:
        md = PR.MdTag(g("mismatchingPositions"), reference_pos)
    except PR.PileupThrow as e:
        raise MdTagRejects(str(e)) from None

    def pileup(reference_base, **events):  # new Pileup(referenceId, referencePos, referenceName, base, ...)
        p = dict(referenceId=need("referenceId"), referencePosition=reference_pos,
                 referenceName=need("referenceName"), referenceBase=reference_base,
                 matches=[], mismatches=[], insertions=[], deletes=[])
        p.update(events)
        return p

    def mapq_qual():  # record.getMapq.toInt, stringToQualitySanger(record.getQual.toString)
        need("mapq")
        need("qual")

    out: List[dict] = []
    for length, op in cigar:
        if op == "I":  # :129-134: one event per element, the whole sequence
            name, seq = need("readName"), need("sequence")
            mapq_qual()
            out.insert(0, pileup(None, insertions=[dict(readName=name, insertedSequence=seq)]))
            read_pos += length
        elif op == "M":  # :137-162
            for _ in range(length):
                if md.is_match(reference_pos):
                    name, rev = need("readName"), need("readNegativeStrand")
                    mapq_qual()
                    ev = dict(readName=name, isReverseStrand=rev)
                    need("referenceId"), need("referenceName")
                    out.insert(0, pileup(base_from_sequence(read_pos), matches=[ev]))
                else:
                    m = md.mismatched_base(reference_pos)
                    if m is None:
                        raise IllegalArgumentException("Cigar match has no MD (mis)match @%d" % reference_pos)
                    name = need("readName")
                    mismatched = base_from_sequence(read_pos)
                    rev = need("readNegativeStrand")
                    mapq_qual()
                    ev = dict(readName=name, mismatchedBase=mismatched, isReverseStrand=rev)
                    need("referenceId"), need("referenceName")
                    out.insert(0, pileup(base_with_name(m), mismatches=[ev]))
                read_pos += 1
                reference_pos += 1
        elif op == "D":  # :165-178
            for _ in range(length):
                d = md.deleted_base(reference_pos)
                if d is None:
                    raise IllegalArgumentException("CIGAR delete but the MD tag is not a delete")
                name = need("readName")
                mapq_qual()
                need("referenceId"), need("referenceName")
                out.insert(0, pileup(base_with_name(d), deletes=[dict(readName=name)]))
                reference_pos += 1
        else:  # :181-187
            if op in PR._CONSUMES_READ:
                read_pos += length
            if op in PR._CONSUMES_REF:
                reference_pos += length
    return out


def traverse(recs: List[dict], f: Callable[[dict], None]) -> None:
    """PileupTraversable.foreach, :194-280, over the records LocusPredicate
    keeps; `f` gets every flushed Pileup.  On top of the Scala's own asserts,
    any decrease of start inside a run of one referenceId raises
    :class:`Unsorted` (the project's declaration)."""
    pileups: Dict[int, List[dict]] = {}  # the SortedMap: flushed in key order
    current_reference: Optional[int] = None
    current_reference_position: Optional[int] = None
    previous_start: Optional[int] = None

    def flush(before: Optional[int] = None):  # :203-241
        locations = sorted(k for k in pileups if before is None or k < before)
        for location in locations:
            matches, mismatches, deletes, inserts = [], [], [], []
            reference_name = None
            reference_base = None
            for p in pileups[location]:
                assert p["referenceId"] == current_reference
                assert p["referencePosition"] == location
                matches += p["matches"]
                mismatches += p["mismatches"]
                deletes += p["deletes"]
                inserts += p["insertions"]
                if reference_name is not None:
                    assert reference_name == p["referenceName"]
                if reference_base is not None and p["referenceBase"] is not None:
                    if reference_base != p["referenceBase"]:  # :230
                        raise ReferenceConflict(p["referenceName"], location)
                reference_name = p["referenceName"]
                if p["referenceBase"] is not None:
                    reference_base = p["referenceBase"]
            f(dict(referenceId=current_reference, referencePosition=location, referenceName=reference_name,
                   referenceBase=reference_base, matches=matches, mismatches=mismatches, insertions=inserts,
                   deletes=deletes))
        for location in locations:
            del pileups[location]

    for i, read in enumerate(recs):
        if read is None or not PR.locus_predicate(read):
            continue
        try:
            ref_id, start = read.get("referenceId"), read.get("start")
            if ref_id is None:  # :248 / :254 unbox
                raise NullPointerException("referenceId")
            if current_reference is not None and current_reference == ref_id:
                if start is None:  # :260
                    raise NullPointerException("start")
                if start < current_reference_position:  # :260, the reference's own assert
                    raise Unsorted("You can only create pileups on sorted BAM/ADAM files")
                if start < previous_start:  # declared: any decrease
                    raise Unsorted("start decreases inside a run of one reference")
            else:
                if current_reference is not None:
                    flush()  # :256
                if start is None:  # :249
                    raise NullPointerException("start")
                current_reference, current_reference_position = ref_id, start
            previous_start = start
            for p in read_to_pileups(read):  # :266-272
                pileups.setdefault(p["referencePosition"], []).append(p)
            flush(start)  # :275
        except ReferenceConflict:
            raise
        except MpileupThrow as e:
            raise type(e)(e.what, i) from None
    flush()  # :279


def line_of(p: dict) -> str:
    """the print loop of MpileupCommand.run, :48-80"""
    num_reads = len(p["matches"]) + len(p["mismatches"]) + len(p["insertions"]) + len(p["deletes"])
    out = ["%s %s " % (p["referenceName"], p["referencePosition"])]
    out.append(p["referenceBase"] if p["referenceBase"] is not None else "?")
    out.append(" %d " % num_reads)
    for ev in p["matches"]:
        out.append("," if ev["isReverseStrand"] else ".")
    for ev in p["mismatches"]:
        out.append(ev["mismatchedBase"].lower() if ev["isReverseStrand"] else ev["mismatchedBase"])
    for _ in p["deletes"]:
        out.append("-1" + p["referenceBase"])
    for ev in p["insertions"]:
        out.append("+%d%s" % (len(ev["insertedSequence"]), ev["insertedSequence"]))
    out.append("\n")
    return "".join(out)


def mpileup(recs: List[dict]) -> str:
    """what `adam mpileup` prints for the records, when nothing throws"""
    lines: List[str] = []
    traverse(recs, lambda p: lines.append(line_of(p)))
    return "".join(lines)


def pileups(recs: List[dict]) -> List[dict]:
    out: List[dict] = []
    traverse(recs, out.append)
    return out
