"""adam_amd.inputs on the host: SamInput's partitions and lifetimes (with a
recording parse in place of sam.SamText), text_output's file rules, and
rebased over every message form the four rebasing commands can meet."""
import io
import os
import types

import pytest

from adam_amd import _capi
from adam_amd.inputs import Phases, SamInput, rebased, sam_partitions, text_output

HEADER = b"@HD\tVN:1.4\n@SQ\tSN:1\tLN:1000\n"
TEXT = HEADER + b"".join(b"r%02d\t0\t1\t%d\t30\t4M\t*\t0\t0\tACGT\tIIII\n" % (k, k + 1) for k in range(40))
PARTITION_BYTES = 200  # five or six records per range


class Parses:
    """parse= for SamInput: records every parse, what was open when it was
    built, and counts the records the way the device parse does"""

    def __init__(self):
        self.made = []

    def __call__(self, data, ctx, bam=False):
        raw = bytes(data)
        p = types.SimpleNamespace(data=raw, bam=bam, closed=False, open_before=[q for q in self.made if not q.closed])
        n = 0 if bam else sum(1 for line in raw.splitlines() if line and not line.startswith(b"@"))
        p.counts = lambda: types.SimpleNamespace(n_reads=n)
        p.close = lambda: setattr(p, "closed", True)
        self.made.append(p)
        return p


@pytest.fixture
def sam_file(tmp_path):
    f = tmp_path / "in.sam"
    f.write_bytes(TEXT)
    return str(f)


def test_partitioned_sam(sam_file):
    header, ranges = sam_partitions(TEXT, PARTITION_BYTES)
    assert header == HEADER and len(ranges) >= 5
    P, ph = Parses(), Phases()
    bases = []
    with SamInput(sam_file, "ctx", ph, PARTITION_BYTES, parse=P) as src:
        assert src.n_partitions == len(ranges) and not src.bam
        for sam, base in src:
            assert sam is P.made[-1] and not sam.closed
            bases.append(base)
    assert [p.data for p in P.made] == [HEADER + TEXT[a:b] for a, b in ranges]
    want, total = [], 0
    for p in P.made:
        want.append(total)
        total += p.counts().n_reads
    assert bases == want and total == 40
    assert all(p.open_before == [] for p in P.made)  # parse k was closed before parse k + 1 was built
    assert all(p.closed for p in P.made)
    assert "parse" in ph.t


@pytest.mark.parametrize("content, partition_bytes, bam", [
    (TEXT, None, False),
    (TEXT, len(TEXT) + 1, False),
    (b"\x1f\x8b\x08\x04" + bytes(24), 4, True),
    (b"", 4, False),
])
def test_whole_input_is_one_parse(tmp_path, content, partition_bytes, bam):
    f = tmp_path / "in"
    f.write_bytes(content)
    P = Parses()
    with SamInput(str(f), None, Phases(), partition_bytes, parse=P) as src:
        assert src.n_partitions == 1 and src.bam is bam
        assert [base for _, base in src] == [0]
    assert [(p.data, p.bam, p.closed) for p in P.made] == [(content, bam, True)]


def test_exception_in_the_loop_body(sam_file):
    P = Parses()
    seen = {}
    try:
        with SamInput(sam_file, None, Phases(), PARTITION_BYTES, parse=P) as src:
            seen["map"] = src.data
            for k, (sam, base) in enumerate(src):
                if k == 1:
                    raise KeyError("body")
    except KeyError:
        # still inside the handler: the traceback, and with it the loop's frame, is alive
        assert len(P.made) == 2 and all(p.closed for p in P.made)
        assert seen["map"].closed
    else:
        pytest.fail("the exception did not leave the block")


def test_two_passes(sam_file):
    _, ranges = sam_partitions(TEXT, PARTITION_BYTES)
    P = Parses()
    with SamInput(sam_file, None, Phases(), PARTITION_BYTES, parse=P) as src:
        first = [base for _, base in src]
        assert all(p.closed for p in P.made)
        second = [base for _, base in src]
    assert first == second and len(P.made) == 2 * len(ranges)
    assert [p.data for p in P.made[:len(ranges)]] == [p.data for p in P.made[len(ranges):]]
    assert all(p.closed and p.open_before == [] for p in P.made)


def partials(d):
    return [n for n in os.listdir(d) if ".partial." in n]


def test_text_output_success(tmp_path):
    out = tmp_path / "o.txt"
    with text_output(str(out)) as sink:
        sink.write(b"ab")
        sink.write(b"c\n")
        assert not out.exists()
    assert out.read_bytes() == b"abc\n" and partials(tmp_path) == []


def test_text_output_exception_after_a_write(tmp_path):
    out = tmp_path / "o.txt"
    with pytest.raises(KeyError):
        with text_output(str(out)) as sink:
            sink.write(b"ab")
            assert len(partials(tmp_path)) == 1
            raise KeyError("late")
    assert os.listdir(tmp_path) == []


def test_text_output_exception_before_any_write(tmp_path):
    out = tmp_path / "o.txt"
    with pytest.raises(KeyError):
        with text_output(str(out)):
            assert os.listdir(tmp_path) == []
            raise KeyError("early")
    assert os.listdir(tmp_path) == []


def test_text_output_clean_exit_without_a_write(tmp_path):
    out = tmp_path / "o.txt"
    with text_output(str(out)):
        pass
    assert out.read_bytes() == b"" and partials(tmp_path) == []


def test_text_output_refuses_a_directory(tmp_path):
    with pytest.raises(IsADirectoryError) as e:
        with text_output(str(tmp_path)):
            pytest.fail("entered")
    assert str(e.value) == "output path %s is a directory" % tmp_path


def test_text_output_stdout():
    buf = io.BytesIO()
    with text_output(None, stdout=buf) as sink:
        sink.write(b"xyz")
    assert buf.getvalue() == b"xyz"


# every fail(...) text with "read N" that flagstat, print_tags, reads2ref and aggregate_pileups can meet
# (flagstat.hip flagstat_end, tags.hip tags_error, adam_out.hip adam_code_fail, pileup.hip pileup_prepare);
# {} is where the read's index goes
MESSAGES = [
    (_capi.NULL_FIELD, "flagstat: read {} has its mate mapped to a different chromosome and a null mapq (the "
                       "reference's getMapq >= 5 throws a NullPointerException)"),
    (_capi.NULL_FIELD, "print_tags: read {} has a null failedVendorQualityChecks or null attributes (the reference "
                       "throws a NullPointerException)"),
    (_capi.ATTRIBUTE, "print_tags: read {} has an attribute AttributeUtils.parseAttribute throws at"),
    (_capi.UNSUPPORTED, "print_tags: read {} has a non-ASCII byte in a tag name or in an A / i / f / H / B value"),
    (_capi.INVALID_ARG, "print_tags: read {}: the attributes offsets leave the column's bytes"),
    (_capi.UNSUPPORTED, "print_tags: read {}: the counted tag's value is of type B (an array the reference keys by "
                        "identity)"),
    (_capi.UNSUPPORTED, "ADAM record of read {}: an H or B tag (the reference's attribute conversion throws)"),
    (_capi.SAM_PARSE, "ADAM record of read {}: an integer / float tag value that does not parse"),
    (_capi.NULL_FIELD, "reads2ref: read {}: a null start, sequence or qual (the reference throws a "
                       "NullPointerException)"),
    (_capi.MD_PARSE, "reads2ref: read {}: an MD tag MdTag.apply rejects"),
    (_capi.UNSUPPORTED, "reads2ref: read {}: beyond the device path's limits (a mismatch or deleted base 2^26 or more "
                        "positions after the read's start, or 2^31 or more rows or read bases in one read)"),
    (_capi.PILEUP, "made up: read {}: 15 of its 5 bases, 55, read 15"),  # the index's digits elsewhere
]


@pytest.mark.parametrize("read", [5, 2, 0, 31])
@pytest.mark.parametrize("status, form", MESSAGES)
def test_rebased(status, form, read):
    e = _capi.BQSRError(status, form.format(read), read)
    assert rebased(e, 0) is e
    r = rebased(e, 1000)
    assert (r.status, r.read) == (status, read + 1000)
    assert str(r) == str(_capi.BQSRError(status, form.format(read + 1000), read + 1000))
    # the two rules this one replaces (print_tags: every "read N"; reads2ref: the first "read N:") agree with it
    msg = str(e).split(": ", 1)[1]
    every = msg.replace("read %d" % read, "read %d" % (read + 1000))
    colon = msg.replace("read %d:" % read, "read %d:" % (read + 1000), 1)
    if "made up" not in form:
        assert str(r).split(": ", 1)[1] == every
        if "read %d:" % read in msg:
            assert every == colon


def test_rebased_leaves_an_error_without_a_read():
    e = _capi.BQSRError(_capi.DEVICE, "hipMalloc failed: out of memory")
    assert rebased(e, 1000) is e
