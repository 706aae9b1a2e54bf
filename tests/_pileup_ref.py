"""`adam reads2ref` restated in plain Python: the yardstick of the pileup tests.

Reads2PileupProcessor.readToPileups (adam-core/.../rdd/Reads2PileupProcessor.
scala:34-197) over MdTag (util/MdTag.scala:38-98, 247-269), RichADAMRecord's
qualityScores and end (rich/RichADAMRecord.scala:43, 77-87) and LocusPredicate
(predicates/LocusPredicate.scala), written from the Scala, statement by
statement, over the ADAMRecord dicts ``_adam_ref.convert_sam`` returns (or
dicts built by hand: a missing key is a null field).  Nothing here knows how
the device does it.

Where the Scala throws, :class:`PileupThrow` carries the status name the C ABI
gives that exception: NULL_FIELD (a NullPointerException on a null start,
sequence or qual), MD_PARSE (MdTag.apply's IllegalArgumentException, toInt's
NumberFormatException included), PILEUP (everything thrown inside the CIGAR
walk: Base.valueOf, substring / array indices, the two CIGAR-against-MD
IllegalArgumentExceptions, the end != -1 assert of an unmapped read).
"""
from __future__ import annotations

import re
from typing import Dict, List, Optional

# adam.avdl:70-88
BASES = ["A", "C", "T", "G", "U", "N", "X", "K", "M", "R", "Y", "S", "W", "B", "V", "H", "D"]
# adam.avdl:99-128
FIELDS = ["referenceName", "referenceId", "position", "rangeOffset", "rangeLength", "referenceBase", "readBase",
          "sangerQuality", "mapQuality", "numSoftClipped", "numReverseStrand", "countAtPosition", "readName",
          "readStart", "readEnd", "recordGroupSequencingCenter", "recordGroupDescription", "recordGroupRunDateEpoch",
          "recordGroupFlowOrder", "recordGroupKeySequence", "recordGroupLibrary",
          "recordGroupPredictedMedianInsertSize", "recordGroupPlatform", "recordGroupPlatformUnit",
          "recordGroupSample"]
RG_FIELDS = FIELDS[15:]

_DIGITS = re.compile(r"[0-9]+")
_MD_BASES = re.compile(r"[AaGgCcTtNnUuKkMmRrSsWwBbVvHhDdXxYy]+")
_CIGAR = re.compile(r"([0-9]+)([MIDNSHP=X])")
_CONSUMES_READ = set("MIS=X")
_CONSUMES_REF = set("MDN=X")


class PileupThrow(Exception):
    def __init__(self, status: str, what: str = "", read: int = -1):
        super().__init__("%s: %s" % (status, what))
        self.status = status
        self.read = read


class MdTag:
    """MdTag.apply(mdTagInput, referenceStart), MdTag.scala:38-98"""

    def __init__(self, md: Optional[str], start: int):
        self.matches: List[range] = []
        self.mismatches: Dict[int, str] = {}
        self.deletes: Dict[int, str] = {}
        if md is None or len(md) == 0:
            return
        md = md.upper()
        end = len(md)
        self.offset = 0
        self.pos = start

        def read_matches(msg):
            m = _DIGITS.match(md, self.offset)
            if m is None:
                raise PileupThrow("MD_PARSE", msg)
            length = int(m.group())
            if length > 2 ** 31 - 1:
                raise PileupThrow("MD_PARSE", "NumberFormatException")
            if length > 0:
                self.matches.insert(0, range(self.pos, self.pos + length))
            self.offset += len(m.group())
            self.pos += length

        read_matches("no leading match count")
        while self.offset < end:
            delete = md[self.offset] == "^"
            if delete:
                self.offset += 1
            m = _MD_BASES.match(md, self.offset)
            if m is None:
                raise PileupThrow("MD_PARSE", "no bases after a match count")
            for base in m.group():
                (self.deletes if delete else self.mismatches)[self.pos] = base
                self.pos += 1
            self.offset += len(m.group())
            read_matches("no match count after bases")

    def is_match(self, pos: int) -> bool:
        return any(pos in r for r in self.matches)

    def mismatched_base(self, pos: int) -> Optional[str]:
        return self.mismatches.get(pos)

    def deleted_base(self, pos: int) -> Optional[str]:
        return self.deletes.get(pos)


def _base_value_of(s: str) -> str:
    """Base.valueOf: the symbol itself, IllegalArgumentException otherwise"""
    if s not in BASES:
        raise PileupThrow("PILEUP", "no Base symbol " + repr(s))
    return s


def decode_cigar(text: str):
    """TextCigarCodec.decode: "*" is the empty CIGAR"""
    if text == "*":
        return []
    return [(int(n), op) for n, op in _CIGAR.findall(text)]


def read_to_pileups(rec: dict) -> List[dict]:
    """readToPileups(record): the read's pileups in the order of the returned
    list (built by prepending: reverse walk order)."""
    g = rec.get
    if g("cigar") is None or g("mismatchingPositions") is None:
        return []
    cigar = decode_cigar(g("cigar"))
    if g("start") is None:  # MdTag(md, referencePos): the boxed start unboxed
        raise PileupThrow("NULL_FIELD", "start")
    start = g("start")
    md = MdTag(g("mismatchingPositions"), start)
    is_reverse = bool(g("readNegativeStrand"))

    def sequence():
        if g("sequence") is None:
            raise PileupThrow("NULL_FIELD", "sequence")
        return g("sequence")

    def base_from_sequence(pos):
        s = sequence()
        if pos + 1 > len(s):  # subSequence(pos, pos + 1)
            raise PileupThrow("PILEUP", "sequence index %d" % pos)
        return _base_value_of(s[pos])

    def populate(reference_pos, read_pos):
        # record.end: None unless readMapped -> -1 -> the assert
        if not g("readMapped"):
            raise PileupThrow("PILEUP", "record.end is None: the read is not mapped")
        end = start + sum(n for n, op in cigar if op in _CONSUMES_REF)
        if g("qual") is None:
            raise PileupThrow("NULL_FIELD", "qual")
        if read_pos >= len(g("qual")):
            raise PileupThrow("PILEUP", "quality index %d" % read_pos)
        q = (ord(g("qual")[read_pos]) - 33) & 0xFF  # .toByte
        row = dict.fromkeys(FIELDS)
        row.update(referenceName=g("referenceName"), referenceId=g("referenceId"), mapQuality=g("mapq"),
                   position=reference_pos, sangerQuality=q - 256 if q >= 128 else q,
                   numReverseStrand=1 if is_reverse else 0, numSoftClipped=0, readName=g("readName"),
                   readStart=start, readEnd=end, countAtPosition=1)
        for f in RG_FIELDS:
            row[f] = g(f)
        return row

    reference_pos, read_pos = start, 0
    out: List[dict] = []
    for length, op in cigar:
        if op == "I":
            s = sequence()
            if read_pos + length > len(s):  # substring(readPos, readPos + length)
                raise PileupThrow("PILEUP", "insert beyond the sequence")
            for insert_pos, b in enumerate(s[read_pos:read_pos + length]):
                base = _base_value_of(b)
                row = populate(reference_pos, read_pos)
                row.update(readBase=base, rangeOffset=insert_pos, rangeLength=length, referenceBase=None)
                out.insert(0, row)
                read_pos += 1
        elif op == "M":
            for _ in range(length):
                if md.is_match(reference_pos):
                    ref = base_from_sequence(read_pos)
                else:
                    m = md.mismatched_base(reference_pos)
                    if m is None:
                        raise PileupThrow("PILEUP", "M base at %d: the MD has neither a match nor a mismatch" % reference_pos)
                    ref = _base_value_of(m)
                row = populate(reference_pos, read_pos)
                row.update(readBase=base_from_sequence(read_pos), referenceBase=ref)
                out.insert(0, row)
                read_pos += 1
                reference_pos += 1
        elif op == "D":
            for i in range(length):
                d = md.deleted_base(reference_pos)
                if d is None:
                    raise PileupThrow("PILEUP", "D base: the MD has no delete there")
                row = populate(reference_pos, read_pos)
                row.update(referenceBase=_base_value_of(d), rangeOffset=i, rangeLength=length)
                out.insert(0, row)
                reference_pos += 1
        elif op == "S":
            for clip_pos in range(length):
                base = base_from_sequence(read_pos)
                row = populate(reference_pos, read_pos)
                row.update(readBase=base, numSoftClipped=1, rangeOffset=clip_pos, rangeLength=length,
                           referenceBase=None)
                out.insert(0, row)
                read_pos += 1
        else:
            if op in _CONSUMES_READ:
                read_pos += length
            if op in _CONSUMES_REF:
                reference_pos += length
    return out


def reads_to_pileups(recs: List[dict]) -> List[dict]:
    """reads.flatMap(readToPileups): reads in input order; the first throwing
    read fails the job (PileupThrow.read = its index)."""
    out: List[dict] = []
    for i, rec in enumerate(recs):
        try:
            out.extend(read_to_pileups(rec))
        except PileupThrow as e:
            raise PileupThrow(e.status, str(e), i) from None
    return out


def locus_predicate(rec: dict) -> bool:
    """LocusPredicate: equalTo on four columns; a null fails"""
    g = rec.get
    return (g("readMapped") is True and g("primaryAlignment") is True and
            g("failedVendorQualityChecks") is False and g("duplicateRead") is False)
