"""The tests' DEFLATE / BGZF writer (_deflate.py) and the crafted members of
test_gpu_bgzf_bytes.py (_bgzf_cases.py) against zlib, without a GPU: every
well-formed stream inflates under zlib to the bytes its token list stands
for, every malformed member makes zlib raise -- so zlib is the reference for
the bytes and for the accept / reject decision the device decoder is held to.
The cases' coverage claims (which alignments, bit offsets, table widths and
repeat codes they reach) are checked here too."""
import zlib

import pytest

import _bgzf_cases as C
import _deflate as D


@pytest.fixture(scope="module")
def groups():
    return {name: make() for name, make in C.GROUPS.items()}


def test_bit_writer_and_canonical_codes():
    w = D.BitWriter()
    w.bits(0b101, 3)
    w.code(0b110, 3)  # (most significant bit first: 1, 1, 0)
    w.bits(0x1FF, 9)
    assert w.bitpos == 15 and w.bytes() == bytes([0b11011101, 0b01111111])
    # RFC 1951 §3.2.2's example
    assert D.canonical([3, 3, 3, 3, 3, 2, 4, 4]) == [(2, 3), (3, 3), (4, 3), (5, 3), (6, 3), (0, 2), (14, 4), (15, 4)]
    assert D.kraft(D.FIXED_LIT) == 32768 and D.kraft(C.LIT15) == 32768 and D.kraft(C.LIT286) == 32768
    assert D.kraft(C.DIST15) == 32768 and D.kraft(C.DIST30) == 32768
    assert [D.length_symbol(n)[0] for n in (3, 10, 11, 257, 258)] == [257, 264, 265, 284, 285]
    assert [D.dist_symbol(n)[0] for n in (1, 4, 5, 24577, 32768)] == [0, 3, 4, 29, 29]


def test_writer_round_trips_zlib_tokens():
    # the writer's fixed and dynamic forms of a long token list, and stored blocks, against zlib
    toks = C.use_all(C.LIT286, D.FIXED_DIST[:30], lead=1)
    want = D.expand(toks)
    for s in (C.Stream().fixed(toks, True), C.Stream().dynamic(toks, C.LIT286, C.DIST30, True),
              C.Stream().dynamic(toks, C.LIT286, C.DIST30, True, rle=True),
              C.Stream().stored(want[:1000]).stored(want[1000:], True)):
        assert zlib.decompress(s.w.bytes(), -15) == want == s.out


@pytest.mark.parametrize("name", sorted(C.GROUPS))
def test_members_against_zlib(groups, name):
    members = groups[name]
    assert len({m.name for m in members if not m.good}) == sum(not m.good for m in members)
    for m in members:
        gz = m.bytes()
        if m.good:
            assert zlib.decompress(m.raw, -15) == m.data, m.name
            assert zlib.decompress(gz, 31) == m.data, m.name
        else:
            with pytest.raises(zlib.error):
                zlib.decompress(gz, 31)
                pytest.fail("zlib accepts " + m.name)
    lay = D.layout(C.pack(members))
    assert len(lay) == len(members)
    for m, (src, csize, dst, isize) in zip(members, lay):
        assert csize == len(m.raw) - m.wrap.get("cut", 0), m.name
        assert isize <= 65536 and (not m.good or isize == len(m.data)), m.name


def test_malformed_deflate_is_malformed_raw(groups):
    # the members whose DEFLATE stream itself is malformed (not only the wrapper's CRC32 / ISIZE / length)
    wrapper_only = ("over-isize", "short-of-isize", "crc-bit", "data-bit", "cut-")
    n = 0
    for m in groups["invalid"] + groups["reader"]:
        if m.good or m.name.startswith(wrapper_only):
            continue
        with pytest.raises(zlib.error):
            zlib.decompress(m.raw, -15)
        n += 1
    assert n >= 25


def test_coverage_of_the_cases(groups):
    by = {g: {m.name: m for m in ms} for g, ms in groups.items()}
    # second-level tables of every width, 15-bit members
    assert C.second_level_widths(C.LIT15, 9) == [1, 2, 3, 4, 5, 6]
    assert C.second_level_widths(C.DIST15, 8) == [7] and max(C.DIST15) == 15
    assert sum(1 << w for w in C.second_level_widths(C.DIST30, 8)) == 134  # (within the decoder's 256)
    # every length and distance symbol at its smallest and largest extra value
    toks = C.use_all(C.FIXED286, D.FIXED_DIST[:30], lead=1)
    lens = {(t[1], t[2]) for t in toks if not isinstance(t, int)}
    dists = {(t[3], t[4]) for t in toks if not isinstance(t, int)}
    for s in range(29):
        assert {(257 + s, 0), (257 + s, (1 << D.LEN_EXTRA[s]) - 1)} <= lens
    for s in range(30):
        assert {(s, 0), (s, (1 << D.DIST_EXTRA[s]) - 1)} <= dists
    data = D.expand(toks)
    assert len(data) > 32768 and {D.DIST_BASE[s] + e for s, e in dists} >= {24577, 32768}
    # the repeat codes at their smallest and largest counts, one running into the distance lengths
    seq = D.cl_rle(C.RLE_LIT + C.RLE_DIST)
    assert [x for x in seq if x[0] >= 16] == C.RLE_WANT
    n = 0
    for s, e in seq:
        k = {16: 3, 17: 3, 18: 11}.get(s, 1) + (e if s >= 16 else 0)
        crosses = n < len(C.RLE_LIT) < n + k
        n += k
        if crosses:
            assert s == 16
            break
    else:
        pytest.fail("no repeat crosses from the literal/length lengths into the distance lengths")
    # stored blocks at the eight bit offsets; the start alignments mod 16; the compressed sizes
    assert sorted(C.stored_bit_offsets()) == list(range(8))
    lay = D.layout(C.pack(groups["reader"]))
    assert {lay[i][0] % 16 for i in range(16)} == set(range(16))
    assert all(groups["reader"][i].raw == groups["reader"][0].raw for i in range(16))
    for n in C.CSIZES:
        assert len(by["reader"]["csize-%d" % n].raw) == n
    assert len(by["reader"]["ends-on-a-byte"].raw) == 8  # (3 + 6 * 9 + 7 bits)
    assert len(by["blocks"]["stored-65505"].bytes()) == 65536
    # the output alignments of the small members
    lay = D.layout(C.pack(groups["isize"]))
    for n in C.SMALL:
        got = {dst % 4 for m, (_, _, dst, isize) in zip(groups["isize"], lay) if m.name == "isize-%d" % n}
        assert got == {0, 1, 2, 3}, n
    assert [m.data.__len__() for m in groups["isize"][:len(C.ISIZES)]] == C.ISIZES


def test_bgzf_member_wrapper():
    raw = C.fix("x", [65, 66]).raw
    gz = D.bgzf_member(raw, b"AB", before=D.subfield(b"AA", b"123"), after=D.subfield(b"ZZ"))
    assert zlib.decompress(gz, 31) == b"AB"
    (src, csize, dst, isize), = D.layout(gz)
    assert gz[src:src + csize] == raw and isize == 2 and len(gz) == 12 + 7 + 6 + 4 + len(raw) + 8
    for kw in ({"crc": 1}, {"isize": 3}, {"cut": 1}):
        with pytest.raises(zlib.error):
            zlib.decompress(D.bgzf_member(raw, b"AB", **kw), 31)
    assert D.layout(C.pack([], eof=True)) == [(18, 2, 0, 0)]
    assert C.pack([], eof=True) == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
