"""Test infrastructure: a plain-Python restatement of `adam print_tags`
(adam-cli/.../cli/PrintTags.scala:61-89) to check the device path
(adam_amd/csrc/tags.hip, adam_amd/print_tags.py).  Not used by the product.

Records are (attributes, failed) pairs: the attributes string as bytes (None =
null) and failedVendorQualityChecks (None = null).  `sam_records` makes them
from tests/_adam_ref.convert_sam's dicts, `table_records` from an Arrow table.

Rules restated, with the reference's file:line:
  filter     !rec.getFailedVendorQualityChecks; null unboxed -> NPE       cli/PrintTags.scala:70
  tags       attributes.split("\\t").filter(_.length > 0).map(parse)      util/AttributeUtils.scala:47-48
             (null attributes -> NPE; rich/RichADAMRecord.scala:46)
  regex      ([^:]{2}):([AifZHB]):(.*), the whole piece                   util/AttributeUtils.scala:28,59-66
             (Java's `.`: not \\n, \\r, U+0085, U+2028, U+2029)
  values     A valueStr(0); i Integer.valueOf; f Float.valueOf; Z the     util/AttributeUtils.scala:87-99
             string; H Byte.valueOf("" + c) per char; B split(",") into
             Float.valueOf (pieces with '.') / Integer.valueOf
  tag counts one (tag, 1) per attribute, summed                           rdd/AdamRDDFunctions.scala:200-209
  values     the first attribute tagged T of the records that have one,   rdd/AdamRDDFunctions.scala:211-229
             counted per distinct value (Map[Any, Long])
  output     "%3s\\t%d", "\\t%10d\\t%s" (value.toString), "Total: %d"      cli/PrintTags.scala:72-88
Integer.valueOf follows Java 7+ (a leading '+' is accepted).  A tag byte >=
0x80, or one inside an A / i / f / H / B value, and a hexadecimal float are
outside what the device path restates: Unsupported.  The line orders are this
build's: tags ascending by bytes; values by descending count, type letter in
the order A i f Z H, value text ascending by bytes.
"""
from __future__ import annotations

import re
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from _adam_ref import java_float_str
from _float_ref import f32_bits_of_decimal

Record = Tuple[Optional[bytes], Optional[bool]]
TYPE_ORDER = "AifZH"


class TagRefError(Exception):
    """What the reference throws (status ATTRIBUTE: IllegalArgumentException &
    co. out of parseAttribute; NULL_FIELD: NullPointerException), or
    UNSUPPORTED; .read = the record's ordinal"""

    def __init__(self, status: str, what: str, read: int = -1):
        super().__init__("%s: %s" % (status, what))
        self.status = status
        self.read = read


_INT = re.compile(rb"[+-]?[0-9]+\Z")
_FLOAT = re.compile(rb"[+-]?(NaN|Infinity|([0-9]+\.?[0-9]*|\.[0-9]+)([eE][+-]?[0-9]+)?[fFdD]?)\Z")
_LINE_END = re.compile("[\n\r\u0085\u2028\u2029]")


def java_int(s: bytes) -> int:
    """Integer.valueOf (Java 7+)"""
    if not _INT.match(s):
        raise TagRefError("ATTRIBUTE", "NumberFormatException: %r" % s)
    v = int(s)
    if not -2 ** 31 <= v < 2 ** 31:
        raise TagRefError("ATTRIBUTE", "NumberFormatException: %r is outside Int" % s)
    return v


def java_float(s: bytes) -> np.float32:
    """Float.valueOf: String.trim (chars <= ' '), decimal forms with an
    optional type suffix, NaN, Infinity; the nearest binary32 of the decimal
    itself (tests/_float_ref.py)"""
    s = s.strip(bytes(range(0x21)))
    if re.match(rb"[+-]?0[xX]", s):
        raise TagRefError("UNSUPPORTED", "a hexadecimal float: %r" % s)
    if not _FLOAT.match(s):
        raise TagRefError("ATTRIBUTE", "NumberFormatException: %r" % s)
    return np.uint32(f32_bits_of_decimal(s)).view(np.float32)  # correctly rounded: no detour over a double


class Attribute:
    """models/Attribute.scala: tag, type letter, and the value as (key, text):
    `key` compares as the reference's Map[Any, Long] key does within a type
    (Float.equals: one NaN, 0.0 != -0.0), `text` is value.toString"""

    def __init__(self, tag: str, typ: str, key, text: str):
        self.tag, self.type, self.key, self.text = tag, typ, key, text


def parse_attribute(piece: bytes) -> Attribute:
    """AttributeUtils.parseAttribute (util/AttributeUtils.scala:59-99)"""
    if any(c >= 0x80 for c in piece[:2]):
        raise TagRefError("UNSUPPORTED", "a non-ASCII tag byte in %r" % piece)
    if len(piece) < 5 or piece[0] == 0x3A or piece[1] == 0x3A or piece[2] != 0x3A or piece[4] != 0x3A \
            or piece[3:4] not in (b"A", b"i", b"f", b"Z", b"H", b"B"):
        raise TagRefError("ATTRIBUTE", "attribute string %r doesn't match format attrTuple:type:value" % piece)
    tag, typ, val = piece[:2].decode("latin-1"), chr(piece[3]), piece[5:]
    if _LINE_END.search(val.decode("utf-8", "replace")):  # `.` does not match it: the regex fails
        raise TagRefError("ATTRIBUTE", "a line terminator inside %r" % piece)
    if typ == "Z":
        return Attribute(tag, typ, val, val.decode("latin-1"))
    if any(c >= 0x80 for c in val):
        raise TagRefError("UNSUPPORTED", "a non-ASCII byte in the value of %r" % piece)
    if typ == "A":
        if not val:
            raise TagRefError("ATTRIBUTE", "StringIndexOutOfBoundsException: %r" % piece)
        return Attribute(tag, typ, val[:1], chr(val[0]))
    if typ == "i":
        v = java_int(val)
        return Attribute(tag, typ, v, str(v))
    if typ == "f":
        f = java_float(val)
        bits = 0x7fc00000 if np.isnan(f) else int(f.view(np.uint32))
        return Attribute(tag, typ, bits, java_float_str(f))
    if typ == "H":
        d = [java_int(bytes([c])) for c in val]  # Byte.valueOf("" + c): "+" and "-" alone are no numbers
        return Attribute(tag, typ, tuple(d), "Vector(%s)" % ", ".join(map(str, d)))
    # B: Java's split drops trailing empty strings; "" stays one empty piece
    parts = [val] if not val else val.rstrip(b",").split(b",") if val.rstrip(b",") else []
    for p in parts:
        java_float(p) if b"." in p else java_int(p)
    return Attribute(tag, typ, object(), "[array]")  # an array: identity is its key


def parse_attributes(s: bytes) -> List[Attribute]:
    """AttributeUtils.parseAttributes (util/AttributeUtils.scala:47-48)"""
    return [parse_attribute(p) for p in s.split(b"\t") if p]


def sam_records(recs: Iterable[dict]) -> List[Record]:
    """(attributes, failed) of convert_sam's record dicts"""
    return [(r["attributes"].encode("latin-1"), r["failedVendorQualityChecks"]) for r in recs]


def table_records(table) -> List[Record]:
    """(attributes, failed) of an Arrow table; an absent column is all null"""
    import pyarrow as pa
    n = table.num_rows
    names = table.column_names
    a = table.column("attributes").cast(pa.binary()).to_pylist() if "attributes" in names else [None] * n
    f = table.column("failedVendorQualityChecks").to_pylist() if "failedVendorQualityChecks" in names else [None] * n
    return list(zip(a, f))


def kept_tags(records: Sequence[Record]) -> List[Tuple[int, bytes, List[Attribute]]]:
    """(ordinal, attributes, parsed attributes) of the kept records; raises at
    the first failing record in input order"""
    out = []
    for i, (attrs, failed) in enumerate(records):
        try:
            if failed is None:
                raise TagRefError("NULL_FIELD", "null failedVendorQualityChecks")
            if failed:
                continue
            if attrs is None:
                raise TagRefError("NULL_FIELD", "null attributes")
            out.append((i, attrs, parse_attributes(attrs)))
        except TagRefError as e:
            raise TagRefError(e.status, str(e), i) from None
    return out


def characterize_tags(records: Sequence[Record]) -> Tuple[Dict[str, int], int]:
    """adamCharacterizeTags (rdd/AdamRDDFunctions.scala:200-209) and filtered.count()"""
    kept = kept_tags(records)
    counts: Dict[str, int] = {}
    for _, _, tags in kept:
        for a in tags:
            counts[a.tag] = counts.get(a.tag, 0) + 1
    return counts, len(kept)


def characterize_tag_values(records: Sequence[Record], tag: str) -> Dict[Tuple[str, str], int]:
    """adamCharacterizeTagValues (rdd/AdamRDDFunctions.scala:211-229): the
    first attribute tagged `tag` of every kept record that has one; {(type
    letter, value.toString): count}"""
    assert len(tag) == 2  # adamFilterRecordsWithTag's assert (:222)
    by_key: Dict[tuple, List] = {}
    for i, _, tags in kept_tags(records):
        a = next((x for x in tags if x.tag == tag), None)
        if a is None:
            continue
        if a.type == "B":
            raise TagRefError("UNSUPPORTED", "a B value under -count", i)
        e = by_key.setdefault((a.type, a.key), [a.text, 0])
        e[1] += 1
    out: Dict[Tuple[str, str], int] = {}
    for (typ, _), (text, c) in by_key.items():
        assert (typ, text) not in out  # value.toString separates the values of one type
        out[(typ, text)] = c
    return out


def print_tags_ref(records: Sequence[Record], list_n: Optional[int] = None, count: Iterable[str] = ()) -> str:
    """The text PrintTags.run prints (cli/PrintTags.scala:72-88), line orders as this build fixes them"""
    kept = kept_tags(records)
    out = []
    if list_n is not None:
        out += [a.decode("latin-1") for _, a, _ in kept[:max(0, list_n)]]
    tags, total = characterize_tags(records)
    to_count = set(count)
    for tag in sorted(tags, key=lambda t: t.encode("latin-1")):
        out.append("%3s\t%d" % (tag, tags[tag]))
        if tag in to_count:
            vals = characterize_tag_values(records, tag)
            order = lambda kv: (-kv[1], TYPE_ORDER.index(kv[0][0]), kv[0][1].encode("latin-1"))  # noqa: E731
            for (typ, text), c in sorted(vals.items(), key=order):
                out.append("\t%10d\t%s" % (c, text))
    out.append("Total: %d" % total)
    return "\n".join(out)
