"""Test infrastructure: the bit patterns and decimal texts the float-text tests
share (tests/test_float_ref.py on the host, tests/test_gpu_float_text.py on the
device), built once from fixed seeds with tests/_float_ref.py's exact arithmetic.

render_set()  65 552 binary32 patterns (16 records of one `f` tag and a 4 096-element
              B:f array): every power of two with its neighbours, subnormals, the
              largest finite values, infinities, NaN payloads, the floats around
              every power of ten, integers around 2^24, values that need all nine
              digits, and seeded random patterns; both signs.
parse_set()   about 4 300 decimal texts: per seeded float its shortest text, the
              17-digit text of its double, the midpoint to the next float written
              out exactly, that text with a 1 appended and with its last digit
              lowered, and the midpoint rounded to 17 and to 20 digits; then the
              edges (long zero runs, 40+ digits, huge exponents, Java's spellings,
              the overflow and underflow ties).
"""
from __future__ import annotations

import functools
import random
from fractions import Fraction
from typing import Dict, List, Tuple

import _float_ref as F

# the three normal powers of two the one-candidate render printed a digit too long
LONG_POWERS = {0x0f800000: "1.2621775E-29", 0x6b000000: "1.5474251E26", 0x6c800000: "1.2379401E27"}
# a 17-digit rounding of a midpoint the one-multiply parse put one float too low
MIDPOINT_17 = (b"2.6217680715490133e-4", 0x398974c7)

N_RENDER = 16 * 4097
OVERFLOW_TIE_EXACT = b"340282356779733661637539395458142568448"  # (2 - 2^-24) * 2^127: from here on Infinity
OVERFLOW_TIE_17 = b"3.4028235677973366e38"                     # its first 17 digits: below it
JUST_BELOW_OVERFLOW = b"340282356779733661637539395458142568447.999"


def exact_digits(v: Fraction) -> Tuple[int, int]:
    """(d, s) with v == d * 10^s, d not a multiple of ten; v a positive dyadic rational"""
    den = v.denominator
    assert den & (den - 1) == 0
    k = den.bit_length() - 1
    d, s = v.numerator * 5 ** k, -k
    while d % 10 == 0:
        d //= 10
        s += 1
    return d, s


def rounded_digits(v: Fraction, p: int) -> Tuple[int, int]:
    """(d, s): v rounded to p significant digits, nearest with ties to even"""
    k = len(str(v.numerator)) - len(str(v.denominator))
    if Fraction(10) ** k > v:
        k -= 1
    s = k - (p - 1)
    q = v / Fraction(10) ** s
    d = q.numerator // q.denominator
    rem = q - d
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and d & 1):
        d += 1
    return d, s


def sci(d: int, s: int, e: str = "e") -> bytes:
    """d * 10^s as d.ddd<e>x"""
    t = str(d)
    return (t[0] + "." + (t[1:] or "0") + e + str(s + len(t) - 1)).encode()


def plain(d: int, s: int) -> bytes:
    """d * 10^s without an exponent"""
    t = str(d)
    if s >= 0:
        return (t + "0" * s).encode()
    if -s < len(t):
        return (t[:s] + "." + t[s:]).encode()
    return ("0." + "0" * (-s - len(t)) + t).encode()


def midpoint_above(bits: int) -> Fraction:
    """half way from a finite non-negative binary32 to the next one up (from the
    largest: to 2^128, the overflow threshold)"""
    assert bits < F.INF
    return F.f32_value(bits) + Fraction(2) ** (max(bits >> 23, 1) - 151)


@functools.lru_cache(maxsize=None)
def render_set() -> Tuple[int, ...]:
    out: List[int] = []

    def both(b):
        out.extend((b, b | 0x80000000))

    for b in LONG_POWERS:
        both(b)
    for e in range(1, 255):                       # every power of two, an ulp either side
        for b in ((e << 23) - 1, e << 23, (e << 23) + 1):
            both(b)
    for b in list(range(1, 301)) + [0x007fffff, 0x00800000, 0x00800001, 0x7f7ffffe, 0x7f7fffff, F.INF, 0]:
        both(b)
    for b in (0x7fc00000, 0x7fc00001, 0x7fffffff, 0x7fe00000, 0x7f800001, 0x7fa00000, 0x7f812345, 0x7fbfffff):
        both(b)                                   # quiet and signalling NaNs
    for k in range(-45, 39):                      # the floats around 10^k
        c = F.f32_bits_of_decimal(b"1e%d" % k)
        for b in range(max(c - 2, 1), c + 3):
            both(b)
    for b in range(0x4b800000 - 8, 0x4b800000 + 17):  # integers around 2^24
        both(b)
    rng = random.Random(20251)
    nine = 0
    while nine < 300:                             # values that need all nine digits
        b = rng.getrandbits(32)
        if (b >> 23) & 0xff != 0xff and b & 0x7fffffff and len(str(F.shortest_digits(b)[0])) == 9:
            out.append(b)
            nine += 1
    structured = len(out)
    while len(out) < N_RENDER:
        out.append(rng.getrandbits(32))
    assert structured < 5000
    return tuple(out)


def render_structured() -> Tuple[int, ...]:
    """the hand-built part of render_set() and some of the random patterns: 4 000"""
    return render_set()[:4000]


@functools.lru_cache(maxsize=None)
def render_texts() -> Dict[int, str]:
    """shortest_text of every pattern of render_set()"""
    return {b: F.shortest_text(b) for b in set(render_set())}


@functools.lru_cache(maxsize=None)
def parse_floats() -> Tuple[int, ...]:
    """600 seeded finite non-zero floats (magnitudes): over every exponent, and some subnormals"""
    rng = random.Random(20252)
    out = [MIDPOINT_17[1] - 1, 0x00000001, 0x007fffff, 0x00800000, 0x3f800000, 0x3f7fffff, 0x7f7ffffe, 0x4b7fffff]
    while len(out) < 560:
        out.append((rng.randrange(1, 255) << 23) | rng.getrandbits(23))
    while len(out) < 600:
        out.append(rng.randrange(1, 1 << 23))
    return tuple(out)


def texts_of(bits: int, negative: bool, spelled_out: bool = False) -> List[bytes]:
    """the seven texts of one float (a magnitude); spelled_out: the exact ones without an exponent, behind
    however many zeros that takes"""
    sign = b"-" if negative else b""
    v, m = F.f32_value(bits), midpoint_above(bits)
    d, s = exact_digits(m)
    form = plain if spelled_out else sci
    return [sign + t for t in (
        F.shortest_text(bits).encode(),
        sci(*rounded_digits(v, 17)),
        form(d, s),
        form(d * 10 + 1, s - 1),
        form(d - 1, s),
        sci(*rounded_digits(m, 17)),
        sci(*rounded_digits(m, 20), e="E"),
    )]


def midpoint_texts() -> List[bytes]:
    """the five midpoint texts of every seeded float"""
    return [t for i, b in enumerate(parse_floats()) for t in texts_of(b, i % 3 == 2, i % 2 == 0)[2:]]


EDGES = [
    MIDPOINT_17[0],
    b"0." + b"0" * 25 + b"1234567e20", b"0." + b"0" * 30 + b"7",  # 25 and more leading zeros
    b"0" * 30 + b"1.5", b"0" * 27 + b"." + b"0" * 27 + b"9e27",
    b"1." + b"0" * 45 + b"1", b"16777217." + b"0" * 40 + b"1", b"16777216.99999999999999999999999999999999999999999",
    b"3." + b"3" * 44, b"1" + b"0" * 39 + b"e-39", b"123456789012345678901234567890123456789012345e-20",
    b"0.1" + b"0" * 50 + b"e1", b"9" * 45 + b"e-7", b"9" * 45 + b"e-6",
    b"1e400", b"1e-400", b"1e99999999", b"1e-99999999", b"0e400", b"0e99999999", b"0.0e-400", b"-0e400",
    b"1" + b"0" * 50 + b"e-400", b"0." + b"0" * 50 + b"1e400", b"1e+38", b"1E-45", b"1e039", b"1e-0045",
    b".5", b"5.", b"+1.5f", b" 1.5D ", b"1.5F", b"1.5d", b"+.5e1", b"-5.e-1", b"1e1f",
    b"Infinity", b"-Infinity", b"+Infinity", b"NaN", b"-NaN", b"+NaN",
    OVERFLOW_TIE_17, OVERFLOW_TIE_EXACT, JUST_BELOW_OVERFLOW, b"3.4028235677973365e38", b"3.4028235677973367e38",
    b"3.4028234e38", b"3.4028235e38", b"3.4028236e38", b"3.4028237e38", b"-3.4028235677973366e38",
    b"-1e-46", b"1e-46", b"7e-46", b"8e-46", b"1.4e-45", b"2.1e-45", b"2.2e-45",
    b"0", b"-0", b"0.0", b"-0.0", b"00", b"0e0",
    b"1.17549435E-38", b"1.17549421E-38", b"1.1754942E-38", b"1.1754943E-38",
]


def underflow_tie() -> bytes:
    """2^-150 written out exactly: half the smallest subnormal"""
    return plain(*exact_digits(Fraction(2) ** -150))


@functools.lru_cache(maxsize=None)
def parse_set() -> Tuple[bytes, ...]:
    out: List[bytes] = []
    for i, b in enumerate(parse_floats()):
        out += texts_of(b, i % 3 == 2, i % 2 == 0)
    tie = underflow_tie()
    out += EDGES + [tie, tie + b"1", b"-" + tie, b"-" + tie + b"1", sci(*exact_digits(Fraction(2) ** -150)),
                    sci(*exact_digits(3 * Fraction(2) ** -150)), sci(*exact_digits(3 * Fraction(2) ** -150)) + b"f"]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def parse_bits() -> Dict[bytes, int]:
    """f32_bits_of_decimal of every text of parse_set()"""
    return {t: F.f32_bits_of_decimal(t) for t in set(parse_set())}


def strtof_reads_alike(t: bytes) -> bool:
    """a text C strtof and Float.parseFloat read the same way: no Java spelling of
    Infinity / NaN, no type suffix, no blanks around"""
    return t.strip(b"+-0123456789.eE") == b""
