"""tests/_float_ref.py pinned: the exact binary32 <-> decimal reference the
device's float text is held to (tests/test_gpu_float_text.py).  Known strings,
the overflow and underflow ties, agreement with numpy's Dragon4
(_adam_ref.java_float_str) on the whole render set, and text -> bits -> text
round trips."""
from fractions import Fraction

import numpy as np
import pytest

import _float_cases as C
import _float_ref as F
from _adam_ref import java_float_str
from _tags_ref import TagRefError, java_float


@pytest.mark.parametrize("bits,text", [
    (0x00000001, "1.4E-45"), (0x7f7fffff, "3.4028235E38"), (0x4b189680, "1.0E7"), (0x4b18967f, "9999999.0"),
    (0x3a83126f, "0.001"), (0x3a83126e, "9.999999E-4"), (0x2edbe6ff, "1.0E-10"), (0x42c80000, "100.0"),
    (0x80000000, "-0.0"), (0x00000000, "0.0"), (0x7f800000, "Infinity"), (0xff800000, "-Infinity"),
    (0x7fc00000, "NaN"), (0xffc00001, "NaN"), (0x7f800001, "NaN"), (0x3f800000, "1.0"), (0xbfc00000, "-1.5"),
    (0x00800000, "1.1754944E-38"), (0x007fffff, "1.1754942E-38"), (0x4b800000, "1.6777216E7"),
] + sorted(C.LONG_POWERS.items()))
def test_known_strings(bits, text):
    assert F.shortest_text(bits) == text
    if text != "NaN":
        assert F.f32_bits_of_decimal(text.encode()) == bits


def test_overflow_tie():
    top = (2 - Fraction(2) ** -24) * Fraction(2) ** 127  # half way from the largest float to 2^128
    assert top == int(C.OVERFLOW_TIE_EXACT) == C.midpoint_above(0x7f7fffff)
    for t in (C.OVERFLOW_TIE_EXACT, C.OVERFLOW_TIE_EXACT + b".000", b"3.40282356779733661637539395458142568448e38",
              b"3.4028235677973367e38", b"3.4028236e38", b"1e39", b"1e99999999"):
        assert F.f32_bits_of_decimal(t) == F.INF, t
        assert F.f32_bits_of_decimal(b"-" + t) == 0xff800000, t
    # the tie cut to 17 digits, 3.4028235677973366e38, is below it (...3366 1637...): the largest float
    assert C.sci(*C.rounded_digits(top, 17)) == C.OVERFLOW_TIE_17 and Fraction(C.OVERFLOW_TIE_17.decode()) < top
    for t in (C.JUST_BELOW_OVERFLOW, C.OVERFLOW_TIE_17, b"3.4028235677973365e38", b"3.4028235e38"):
        assert F.f32_bits_of_decimal(t) == 0x7f7fffff, t


def test_underflow_tie():
    tie = C.underflow_tie()
    assert Fraction(tie.decode()) == Fraction(2) ** -150 and len(tie) > 100
    assert F.f32_bits_of_decimal(tie) == 0 and F.f32_bits_of_decimal(b"-" + tie) == 0x80000000
    assert F.f32_bits_of_decimal(tie + b"1") == 1 and F.f32_bits_of_decimal(b"-" + tie + b"1") == 0x80000001
    assert F.f32_bits_of_decimal(b"-1e-46") == 0x80000000 and F.f32_bits_of_decimal(b"1e-99999999") == 0
    # three halves of the smallest subnormal: a tie between 1 and 2, to the even one
    assert F.f32_bits_of_decimal(C.sci(*C.exact_digits(3 * Fraction(2) ** -150))) == 2


def test_grammar():
    for t, bits in ((b".5", 0x3f000000), (b"5.", 0x40a00000), (b"+1.5f", 0x3fc00000), (b" 1.5D ", 0x3fc00000),
                    (b"\t1e1F\n", 0x41200000), (b"-NaN", F.NAN), (b"+Infinity", F.INF), (b"0e400", 0),
                    (b"-0e99999999", 0x80000000), (b"0" * 30 + b"1.5", 0x3fc00000)):
        assert F.f32_bits_of_decimal(t) == bits, t
    for t in (b"", b".", b"e5", b"1e", b"1e+", b"1.5x", b"0x1p3", b"Inf", b"nan", b"infinity", b"1 .5", b"1.5ff",
              b"--1", b"1.2.3", b"Infinityf"):
        with pytest.raises(ValueError):
            F.f32_bits_of_decimal(t)


def test_named_midpoint_text():
    text, bits = C.MIDPOINT_17
    assert F.f32_bits_of_decimal(text) == bits and text in C.parse_set()
    # the float is 0.00026217682170681655; a double holds the text as the midpoint below it, and rounds it away
    v = F.f32_value(bits)
    assert C.sci(*C.rounded_digits(v, 20)) == b"2.6217682170681655407e-4"
    assert int(np.float32(float(text)).view(np.uint32)) == bits - 1
    assert Fraction(text.decode()) > C.midpoint_above(bits - 1)


def test_shortest_text_against_dragon4():
    """numpy's Dragon4 (unique digits) and the interval rule agree on every pattern of the render set"""
    rs = C.render_set()
    assert len(rs) == C.N_RENDER and set(C.LONG_POWERS) <= set(rs)
    arr = np.array(sorted(set(rs)), dtype=np.uint32)
    texts = C.render_texts()
    for b, f in zip(arr.tolist(), arr.view(np.float32)):
        assert texts[b] == java_float_str(f), hex(b)


def test_text_reads_back():
    for b, t in C.render_texts().items():
        assert F.f32_bits_of_decimal(t.encode()) == (F.NAN if t == "NaN" else b), hex(b)


def test_shortest_text_is_inside_and_minimal():
    """on the structured patterns: the decimal lies inside rounding_interval, and no decimal of fewer digits does"""
    for b in C.render_structured():
        if (b >> 23) & 0xff == 0xff or not b & 0x7fffffff:
            continue
        d, s = F.shortest_digits(b)
        lo, hi, closed = F.rounding_interval(b)
        c = d * Fraction(10) ** s
        assert lo <= c <= hi and (closed or lo < c < hi), hex(b)
        p = len(str(d))
        if p > 2:  # the decimals of p - 1 digits next to the value: both outside (two digits are the least)
            unit = Fraction(10) ** (s + 1)
            q = F.f32_value(b) / unit
            down = q.numerator // q.denominator
            for c in (down * unit, (down + 1) * unit):
                assert not (lo < c < hi) and not (closed and c in (lo, hi)), hex(b)


def test_parse_set_midpoints_go_to_the_even_neighbour():
    want = C.parse_bits()
    assert 4000 <= len(C.parse_set()) <= 4600
    odd = 0
    for i, b in enumerate(C.parse_floats()):
        t = C.texts_of(b, i % 3 == 2, i % 2 == 0)
        sign = 0x80000000 if i % 3 == 2 else 0
        even = b if not b & 1 else b + 1
        odd += b & 1
        assert [want[x] for x in t[:5]] == [sign | b, sign | b, sign | even, sign | (b + 1), sign | b], hex(b)
        assert {want[t[5]], want[t[6]]} <= {sign | b, sign | (b + 1)}
    assert 200 < odd < 400
    # texts of at least 40 digits and of at least 25 leading zeros are there
    digits = lambda t: t.lstrip(b"-").lower().split(b"e")[0].replace(b".", b"").strip(b"0")  # noqa: E731
    assert sum(len(digits(t)) >= 40 for t in C.parse_set()) > 500
    assert sum(t.lstrip(b"-").startswith(b"0." + b"0" * 25) for t in C.parse_set()) > 50


def test_tags_oracle_reads_floats_once():
    """_tags_ref.java_float is the exact parse: no detour over a double"""
    for t, bits in C.parse_bits().items():
        got = java_float(t)
        assert got.dtype == np.float32
        assert int(got.view(np.uint32)) == bits or (bits == F.NAN and np.isnan(got)), t
    for t in (b"abc", b"", b"1e", b"Inf"):
        with pytest.raises(TagRefError) as e:
            java_float(t)
        assert e.value.status == "ATTRIBUTE"
    with pytest.raises(TagRefError) as e:
        java_float(b"0x1p3")
    assert e.value.status == "UNSUPPORTED"
