"""Test infrastructure: exact binary32 <-> decimal text, in integers and
fractions.Fraction only (no float(), no numpy on the value path).  The yardstick
for samk::java_parse_float and samk::java_float_text (adam_amd/csrc/sam_ingest.hip).
Not used by the product.

f32_bits_of_decimal  the correctly rounded binary32 of a decimal string (nearest,
                     ties to even), as Float.parseFloat gives it: any number of
                     digits, gradual underflow, Infinity from (2 - 2^-24) * 2^127
                     up, a signed zero from 2^-150 down.
shortest_text        the fewest significant digits p (at most 9) for which some
                     p-digit decimal lies inside the float's rounding interval
                     (ends included exactly when the mantissa is even, the lower
                     half narrower at a power of two); among those the one nearest
                     the value; laid out as Float.toString lays it out.  The text
                     always shows two digits ("d.d"), so p starts at 2: where one
                     digit would do, the nearest two-digit decimal is taken, as
                     Float.toString's contract has it (Float.MIN_VALUE is 1.4E-45,
                     not 1.0E-45).  That differs from one digit and a 0 only for
                     the smallest subnormals.
"""
from __future__ import annotations

import re
from fractions import Fraction
from typing import Tuple

_WS = bytes(range(0x21))  # String.trim: chars <= ' '
_FLOAT = re.compile(rb"([+-]?)(NaN|Infinity|(?:([0-9]+)\.?([0-9]*)|\.([0-9]+))(?:[eE]([+-]?[0-9]+))?[fFdD]?)\Z")

NAN = 0x7fc00000
INF = 0x7f800000


def round_to_f32(v: Fraction) -> int:
    """bits of the binary32 nearest the non-negative v, ties to even"""
    if v == 0:
        return 0
    e2 = v.numerator.bit_length() - v.denominator.bit_length()  # 2^(e2-1) < v < 2^(e2+1)
    if Fraction(2) ** e2 > v:
        e2 -= 1                                                   # 2^e2 <= v < 2^(e2+1)
    eb = max(e2, -126)
    q = v / Fraction(2) ** (eb - 23)                              # in units of the float grid there
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    return min(((eb + 126) << 23) + n, INF)                       # (a carry out of n lands in the exponent)


def f32_bits_of_decimal(text: bytes) -> int:
    """Float.parseFloat(text) as bits; ValueError where it throws NumberFormatException"""
    s = text.strip(_WS)
    m = _FLOAT.match(s)
    if not m:
        raise ValueError("NumberFormatException: %r" % text)
    sign = 0x80000000 if m.group(1) == b"-" else 0
    if m.group(2) == b"NaN":
        return NAN
    if m.group(2) == b"Infinity":
        return sign | INF
    ip, fp = (m.group(3), m.group(4)) if m.group(3) is not None else (b"", m.group(5))
    digits = (ip + fp).lstrip(b"0")
    mant = int(digits) if digits else 0
    if mant == 0:
        return sign
    e10 = int(m.group(6) or b"0") - len(fp)
    # 10^(top-1) <= value < 10^top: outside [1e-47, 1e40) no power of ten needs writing out
    top = len(digits) + e10
    if top > 40:
        return sign | INF
    if top < -46:
        return sign
    return sign | round_to_f32(Fraction(mant) * Fraction(10) ** e10)


def f32_value(bits: int) -> Fraction:
    """the value of a finite binary32, sign dropped"""
    ef, mf = (bits >> 23) & 0xff, bits & 0x7fffff
    assert ef != 0xff
    return Fraction(mf | 0x800000, 1) * Fraction(2) ** (ef - 150) if ef else Fraction(mf) * Fraction(2) ** -149


def rounding_interval(bits: int) -> Tuple[Fraction, Fraction, bool]:
    """(lo, hi, ends included) of a finite non-zero binary32, sign dropped: the
    reals that round to it"""
    ef, mf = (bits >> 23) & 0xff, bits & 0x7fffff
    v = f32_value(bits)
    ulp = Fraction(2) ** (max(ef, 1) - 150)
    below = ulp / 2 if mf == 0 and ef > 1 else ulp  # a power of two: the floats below are twice as dense
    return v - below / 2, v + ulp / 2, mf & 1 == 0


def shortest_digits(bits: int) -> Tuple[int, int]:
    """(d, s): the decimal d * 10^s of shortest_text, d without trailing zeros (it may have one digit)"""
    # in integers (rounding_interval's numbers times four): v = V * 2^a / 4, the interval [LO, HI] * 2^a / 4
    ef, mf = (bits >> 23) & 0xff, bits & 0x7fffff
    assert ef != 0xff and (ef or mf)
    m = mf | 0x800000 if ef else mf
    a = max(ef, 1) - 150
    V, LO, HI = 4 * m, 4 * m - (1 if mf == 0 and ef > 1 else 2), 4 * m + 2
    closed = m & 1 == 0
    two = 2 ** max(a, 0), 2 ** max(-a, 0)

    def sides(c, s, x):                             # c * 10^s and x * 2^a / 4 over one denominator
        return 4 * c * 10 ** max(s, 0) * two[1], x * two[0] * 10 ** max(-s, 0)

    def inside(c, s):
        l, lo = sides(c, s, LO)
        h, hi = sides(c, s, HI)
        return (lo <= l and h <= hi) if closed else (lo < l and h < hi)

    k = len(str(m)) - 1 + (a * 30103) // 100000     # within one of floor(log10 v)
    while sides(1, k, V)[0] > sides(1, k, V)[1]:
        k -= 1
    while sides(1, k + 1, V)[0] <= sides(1, k + 1, V)[1]:
        k += 1                                      # 10^k <= v < 10^(k+1)
    for p in range(2, 10):
        s = k - (p - 1)
        unit, num = sides(1, s, V)
        down = num // unit
        up = down if down * unit == num else down + 1
        order = [down, up] if 2 * num < (down + up) * unit or (2 * num == (down + up) * unit and not down & 1) \
            else [up, down]                         # the nearer first (a tie: the even one)
        for d in order:
            if inside(d, s):
                while d % 10 == 0:
                    d //= 10
                    s += 1
                return d, s
    raise AssertionError("nine digits always suffice for a binary32: %#x" % bits)


def shortest_text(bits: int) -> str:
    """Float.toString's layout of shortest_digits"""
    bits &= 0xffffffff
    ef, mf = (bits >> 23) & 0xff, bits & 0x7fffff
    if ef == 0xff and mf:
        return "NaN"
    sign = "-" if bits >> 31 else ""
    if ef == 0xff:
        return sign + "Infinity"
    if not bits & 0x7fffffff:
        return sign + "0.0"
    d, s = shortest_digits(bits)
    digits = str(d)
    e = s + len(digits) - 1                         # the first digit's power of ten
    if -3 <= e < 7:                                 # 1e-3 <= |f| < 1e7
        if e >= 0:
            return sign + digits[:e + 1].ljust(e + 1, "0") + "." + (digits[e + 1:] or "0")
        return sign + "0." + "0" * (-e - 1) + digits
    return sign + digits[0] + "." + (digits[1:] or "0") + "E" + str(e)
