"""The print_tags restatement (tests/_tags_ref.py) and the formatter
(adam_amd/print_tags.format_tags), pinned on the reference's own suites and on
a hand-written input whose counts and lines are worked out below --
independently of the device (tests/test_gpu_print_tags.py compares the device
with the restatement)."""
import os

import pytest

from _adam_ref import convert_sam
from _tags_ref import (TagRefError, characterize_tag_values, characterize_tags, parse_attributes, print_tags_ref,
                       sam_records)
from adam_amd.print_tags import _tag_bytes, format_tags, value_order

GOLD = os.path.join(os.path.dirname(__file__), "golden", "reference_resources")


def kept(*attrs):
    return [(a, False) for a in attrs]


# ---- AttributeUtilsSuite (adam-core/src/test/.../util/AttributeUtilsSuite.scala:26-56) ----

def test_parse_tags_returns_a_reasonable_set_of_tag_strings():
    tags = parse_attributes(b"XT:i:3\tXU:Z:foo,bar")
    assert len(tags) == 2
    assert (tags[0].tag, tags[0].type, tags[0].key) == ("XT", "i", 3)
    assert (tags[1].tag, tags[1].type, tags[1].key) == ("XU", "Z", b"foo,bar")


def test_empty_string_is_parsed_as_zero_tag_strings():
    assert parse_attributes(b"") == []


def test_incorrectly_formatted_tag_throws_an_exception():
    with pytest.raises(TagRefError) as e:
        parse_attributes(b"XT:i")
    assert e.value.status == "ATTRIBUTE"


def test_string_tag_with_a_colon_in_it_is_correctly_parsed():
    tags = parse_attributes(b"XX:Z:foo:bar")
    assert len(tags) == 1
    assert tags[0].key == b"foo:bar" and tags[0].text == "foo:bar"


# ---- AdamRDDFunctionsSuite's tag tests (adam-core/src/test/.../rdd/AdamRDDFunctionsSuite.scala:485-547) ----

def test_characterize_tags_counts_integer_tag_values_correctly():
    want = {"XT": 10, "XU": 9, "XV": 8}
    recs = kept(*[b"%s:i:%d" % (t.encode(), i) for t, c in want.items() for i in range(c)])
    assert characterize_tags(recs) == (want, 27)


R4 = kept(b"XX:i:3", b"XX:i:4\tYY:i:10", b"YY:i:20", b"XX:i:4")


def test_with_tag_returns_only_those_records_which_have_the_tag():
    # adamFilterRecordsWithTag("XX") of r1 r2 r3: r1 and r2 -- the records that contribute a value
    assert sum(characterize_tag_values(R4[:3], "XX").values()) == 2
    assert characterize_tag_values(R4[:3], "XX") == {("i", "3"): 1, ("i", "4"): 1}


def test_with_tag_given_a_tag_that_does_not_exist_returns_nothing():
    assert characterize_tag_values(R4[:3], "ZZ") == {}


def test_characterize_tag_values_counts_distinct_values_of_a_tag():
    v = characterize_tag_values(R4, "XX")
    assert len(v) == 2
    assert v[("i", "4")] == 2 and v[("i", "3")] == 1


def test_characterize_tags_counts_tags_in_a_sam_file_correctly():
    recs = sam_records(convert_sam(open(os.path.join(GOLD, "reads12.sam"), "rb").read()))
    counts, total = characterize_tags(recs)
    assert counts["NM"] == 200 and counts["AS"] == 200 and counts["XS"] == 200
    assert total == 200


# ---- a hand-written input ----------------------------------------------------

RECORDS = [
    (b"XT:i:3\tXU:Z:foo,bar", False),          # r0
    (b"XT:i:07\t\tXA:A:c\tXT:i:9", False),     # r1: XT twice (counted twice, value 07 = 7), an empty piece
    (b"XT:i", True),                           # r2: QC-failed -- its malformed attribute is never parsed
    (b"XT:i:7\tXF:f:0.0", False),              # r3
    (b"XT:Z:7\tXF:f:-0.0\tXH:H:0190", False),  # r4: 7 as a string; -0.0 is not 0.0 (Float.equals)
    (b"XT:A:7\tXF:f:NaN\tXB:B:1,2.5", False),  # r5: 7 as a char; a B array of an int and a float
    (b"XF:f:1e10\tXH:H:", False),              # r6: 1.0E10; an empty H
    (None, True),                              # r7: QC-failed -- its null attributes are never read
    (b"", False),                              # r8: no tags
    (b"XF:f:NaN\tXT:i:+3", False),             # r9: NaN equals NaN; +3 = 3 (Java 7+)
    (b"XF:f:0.0\tXT:H:7", False),              # r10: 7 as a byte sequence
]
# kept: every record but r2 and r7
TOTAL = 9
TAGS = {
    "XT": 8,  # r0, r1 twice, r3, r4, r5, r9, r10
    "XU": 1,  # r0
    "XA": 1,  # r1
    "XF": 6,  # r3 r4 r5 r6 r9 r10
    "XH": 2,  # r4 r6
    "XB": 1,  # r5
}
# the first XT of each record: r0 i 3, r1 i 7, r3 i 7, r4 Z "7", r5 A '7', r9 i 3, r10 H [7]
XT = {("i", "3"): 2, ("i", "7"): 2, ("Z", "7"): 1, ("A", "7"): 1, ("H", "Vector(7)"): 1}
# r3 0.0, r4 -0.0, r5 NaN, r6 1.0E10, r9 NaN, r10 0.0
XF = {("f", "0.0"): 2, ("f", "NaN"): 2, ("f", "-0.0"): 1, ("f", "1.0E10"): 1}
XH = {("H", "Vector(0, 1, 9, 0)"): 1, ("H", "Vector()"): 1}
# tags ascending by bytes; values by descending count, then A i f Z H, then text by bytes:
# XF: "0.0" < "NaN" ('0' < 'N') at 2, "-0.0" < "1.0E10" ('-' < '1') at 1;
# XH: "Vector()" < "Vector(0, ..." (')' < '0'); XT: i 3, i 7 at 2, then A, Z, H at 1
TEXT = "\n".join([
    "XT:i:3\tXU:Z:foo,bar",
    "XT:i:07\t\tXA:A:c\tXT:i:9",
    "XT:i:7\tXF:f:0.0",
    " XA\t1",
    " XB\t1",
    " XF\t6",
    "\t         2\t0.0",
    "\t         2\tNaN",
    "\t         1\t-0.0",
    "\t         1\t1.0E10",
    " XH\t2",
    "\t         1\tVector()",
    "\t         1\tVector(0, 1, 9, 0)",
    " XT\t8",
    "\t         2\t3",
    "\t         2\t7",
    "\t         1\t7",
    "\t         1\t7",
    "\t         1\tVector(7)",
    " XU\t1",
    "Total: 9",
])
COUNT = ("XT", "XF", "XH", "ZZ", "toolong")  # ZZ and toolong are no tags of the input: ignored


def test_hand_written_counts():
    assert characterize_tags(RECORDS) == (TAGS, TOTAL)
    assert characterize_tag_values(RECORDS, "XT") == XT
    assert characterize_tag_values(RECORDS, "XF") == XF
    assert characterize_tag_values(RECORDS, "XH") == XH
    assert characterize_tag_values(RECORDS, "XU") == {("Z", "foo,bar"): 1}
    assert characterize_tag_values(RECORDS, "XA") == {("A", "c"): 1}
    assert characterize_tag_values(RECORDS, "ZZ") == {}
    with pytest.raises(TagRefError) as e:  # an array is keyed by identity
        characterize_tag_values(RECORDS, "XB")
    assert (e.value.status, e.value.read) == ("UNSUPPORTED", 5)


def test_hand_written_text():
    assert print_tags_ref(RECORDS, list_n=3, count=COUNT) == TEXT
    # the product's formatter over the same numbers
    lines = [a.decode() for a, f in RECORDS if not f][:3]
    assert format_tags(lines, TAGS, {"XT": XT, "XF": XF, "XH": XH}, TOTAL) == TEXT
    # -list 0 and below print nothing; without -list and -count only the tag lines
    tail = [l for l in TEXT.split("\n")[3:] if not l.startswith("\t")]
    assert print_tags_ref(RECORDS, list_n=0) == "\n".join(tail) == print_tags_ref(RECORDS, list_n=-1)
    assert print_tags_ref(RECORDS) == format_tags([], TAGS, {}, TOTAL) == "\n".join(tail)


def test_value_order():
    items = [(("H", "Vector(7)"), 1), (("Z", "7"), 1), (("i", "7"), 2), (("A", "7"), 1), (("i", "3"), 2),
             (("f", "9.0"), 1), (("i", "10"), 1), (("i", "9"), 1)]
    assert [k for k, _ in sorted(items, key=value_order)] == [
        ("i", "3"), ("i", "7"), ("A", "7"), ("i", "10"), ("i", "9"), ("f", "9.0"), ("Z", "7"), ("H", "Vector(7)")]


@pytest.mark.parametrize("attrs,status", [
    (b"X:i:1", "ATTRIBUTE"),           # a one-char tag
    (b"X::i:1", "ATTRIBUTE"),          # a tag containing ':'
    (b"XT:x:1", "ATTRIBUTE"),          # a type letter outside AifZHB
    (b"XT:A:", "ATTRIBUTE"),           # valueStr(0) of ""
    (b"XT:i:1x", "ATTRIBUTE"),
    (b"XT:i:2147483648", "ATTRIBUTE"),
    (b"XT:i:", "ATTRIBUTE"),
    (b"XT:f:abc", "ATTRIBUTE"),
    (b"XT:H:1A", "ATTRIBUTE"),         # Byte.valueOf("A")
    (b"XT:B:c,1,2", "ATTRIBUTE"),      # the SAM-style subtype letter is no number
    (b"XT:B:", "ATTRIBUTE"),           # "".split(",") is one empty piece
    (b"XT:B:1,,2", "ATTRIBUTE"),
    (b"XT:Z:a\nb", "ATTRIBUTE"),       # `.` stops at a line terminator
    (b"XT:Z:a\xc2\x85b", "ATTRIBUTE"),  # U+0085
    (b"XT:Z:a\xe2\x80\xa8", "ATTRIBUTE"),  # U+2028
    (b"X\xc3\xa9:Z:v", "UNSUPPORTED"),  # a non-ASCII tag
    (b"XT:i:\xd9\xa1", "UNSUPPORTED"),  # an Arabic-Indic digit: Java parses it
    (b"XT:f:0x1p3", "UNSUPPORTED"),    # a hexadecimal float: Java parses it
])
def test_attributes_the_reference_throws_at(attrs, status):
    with pytest.raises(TagRefError) as e:
        characterize_tags(kept(b"XX:i:1") + kept(attrs))
    assert (e.value.status, e.value.read) == (status, 1)
    assert characterize_tags(kept(b"XX:i:1") + [(attrs, True)]) == ({"XX": 1}, 1)  # QC-failed: not parsed


@pytest.mark.parametrize("attrs,tags", [
    (b"XT:B:1,2.5", {"XT": 1}),
    (b"XT:B:,", {"XT": 1}),            # split drops trailing empty strings: no pieces
    (b"XT:B:1,2,,", {"XT": 1}),
    (b"XT:Z:", {"XT": 1}),
    (b"XT:Z:\xc3\xa9\x85", {"XT": 1}),  # any bytes in a Z value; a lone 0x85 is not U+0085
    (b"\x01\x7f:i:1\t ~:A:ab", {"\x01\x7f": 1, " ~": 1}),  # [^:] takes control characters
    (b"XT:f: 1.5f ", {"XT": 1}),       # Float.valueOf trims and takes a type suffix
    (b"XT:i:-2147483648\tXT:i:+2147483647", {"XT": 2}),
    (b"\t\tXT:i:1\t\t", {"XT": 1}),
])
def test_attributes_the_reference_takes(attrs, tags):
    assert characterize_tags(kept(attrs)) == (tags, 1)


def test_null_fields():
    for recs, read in (([(b"", False), (b"", None)], 1), ([(None, False)], 0), ([(None, None)], 0)):
        with pytest.raises(TagRefError) as e:
            characterize_tags(recs)
        assert (e.value.status, e.value.read) == ("NULL_FIELD", read)


def test_tag_name_length():
    assert _tag_bytes("NM") == b"NM"
    for t in ("", "N", "NMX"):
        with pytest.raises(ValueError):
            _tag_bytes(t)
