"""The plain-Python restatement of `adam mpileup` (tests/_mpileup_ref.py) pinned
on facts derived by hand from the fixtures, and what of adam_amd.mpileup and
its C ABI needs no device: argument handling, refusals, the exported symbols."""
import ctypes
import os

import pytest

import _adam_ref
import _mpileup_gen as MG
import _mpileup_ref as MR
from adam_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = os.path.join(ROOT, "tests", "golden", "reference_resources")
NAME = "gi|371561095|gb|CM001014.2|"
SYMBOLS = {"bqsr_sam_mpileup_prepare", "bqsr_sam_mpileup_text", "bqsr_arrow_mpileup_prepare",
           "bqsr_arrow_mpileup_text", "bqsr_mpileup_kernel_times"}


def text_of(name):
    with open(os.path.join(RES, name), "rb") as fh:
        return MR.mpileup(_adam_ref.convert_sam(fh.read()))


@pytest.fixture(scope="module")
def targets():
    return text_of("small_realignment_targets.sam").splitlines()


def test_small_realignment_targets_lines(targets):
    assert len(targets) == 704
    assert targets[0] == NAME + " 701292 T 1 ."
    # the three I elements share their position with the next M base
    assert [l.split(" ")[1] for l in targets if l.split(" ")[3] == "2"] == \
        [l.split(" ")[1] for l in targets if "+" in l] and sum("+" in l for l in targets) == 3
    assert all(l.split(" ")[3] in ("1", "2") for l in targets)


def test_small_realignment_targets_events(targets):
    by_pos = {int(l.split(" ")[1]): l for l in targets}
    assert by_pos[701384] == NAME + " 701384 T 1 G"      # forward mismatch
    assert by_pos[702257] == NAME + " 702257 G 1 c"      # reverse mismatch, reference base from the MD
    assert by_pos[702289] == NAME + " 702289 T 1 -1T"
    ins = by_pos[702323]
    assert ins.startswith(NAME + " 702323 T 2 ,+100CTGTTCGG") and ins.endswith("AGAC")
    assert len(ins) == len(NAME + " 702323 T 2 ,+100") + 100  # a match, then the whole 100-base read
    assert by_pos[869644] == NAME + " 869644 G 1 -1G"
    assert [by_pos[869644 + k].split(" ", 2)[2] for k in (1, 2, 3)] == ["C 1 -1C", "T 1 -1T", "C 1 -1C"]


def test_overlapping_reads():
    lines = text_of("artificial.realigned.sam").splitlines()
    assert lines
    pos = [int(l.split(" ")[1]) for l in lines]
    assert pos == sorted(set(pos))
    deep = 0
    for l in lines:
        name, p, base, count, events = l.split(" ")
        # events: one char per match / mismatch, "-1B" per delete, "+<len><seq>" per insertion
        n, i = 0, 0
        while i < len(events):
            if events[i] == "-":
                i += 3
            elif events[i] == "+":
                j = i + 1
                while events[j].isdigit():
                    j += 1
                i = j + int(events[i + 1:j])
            else:
                i += 1
            n += 1
        assert n == int(count)
        deep += n > 1
    assert deep


def test_unsorted_fixture_is_refused():
    with open(os.path.join(RES, "small.sam"), "rb") as fh:
        recs = _adam_ref.convert_sam(fh.read())
    with pytest.raises(MR.Unsorted) as e:
        MR.mpileup(recs)
    assert e.value.status == "UNSORTED" and e.value.read == 4


def test_restatement_declared_cases():
    # a decrease above the segment's first start: the reference would print positions twice
    recs = MG.records(MG.sam_text([(10, "5M"), (20, "5M"), (15, "5M")]))
    with pytest.raises(MR.Unsorted) as e:
        MR.mpileup(recs)
    assert e.value.read == 2
    # a match on read base N under another read's A
    recs = MG.records(MG.sam_text([(10, "1M", dict(seq="N", md="1")), (10, "1M", dict(seq="A", md="1"))]))
    with pytest.raises(MR.ReferenceConflict) as e:
        MR.mpileup(recs)
    assert (e.value.reference_name, e.value.position) == ("c1", 10)
    # an insertion-only position prints '?'; a reference that comes back is a new segment
    t = MR.mpileup(MG.records(MG.sam_text([(10, "2M1I", dict(rname="c1", flag=16, seq="AAC", md="2", mismatch=0)),
                                           (3, "1M", dict(rname="c2", flag=32, seq="G", md="1")),
                                           (10, "1M", dict(rname="c1", flag=32, seq="A", md="1"))])))
    assert t == "c1 10 A 1 ,\nc1 11 A 1 ,\nc1 12 ? 1 +3AAC\nc2 3 G 1 .\nc1 10 A 1 .\n"


# ---- adam_amd.mpileup without a device -----------------------------------------

def test_cli_arguments(tmp_path, capsys):
    from adam_amd import mpileup as M
    for argv in ([], [str(tmp_path / "absent.sam")], [os.path.join(RES, "small.sam"), "-window_bytes", "0"],
                 [os.path.join(RES, "small.sam"), "-window_bytes", "x"], [os.path.join(RES, "small.sam"), "-bogus"]):
        with pytest.raises(SystemExit) as e:
            M.main(argv)
        assert e.value.code == 2
    capsys.readouterr()


def test_refusals_before_the_device(tmp_path):
    from adam_amd import mpileup as M
    with pytest.raises(ValueError):
        M.mpileup(os.path.join(RES, "small.sam"), window_bytes=0)
    with pytest.raises(IsADirectoryError):
        M.mpileup(os.path.join(RES, "small.sam"), out=str(tmp_path))

    class NoMarkdupColumns:
        markdup = False
    with pytest.raises(ValueError, match="markdup=True"):
        M.arrow_prepare(NoMarkdupColumns())
    assert M.PROJECTION[-4:] == M.LOCUS_COLUMNS and "mismatchingPositions" in M.PROJECTION


def test_new_symbols_and_statuses():
    from adam_amd import mpileup as M
    assert SYMBOLS <= set(_capi.EXPORTS)
    lib = ctypes.CDLL(_capi.LIB_PATH)
    assert all(hasattr(lib, n) for n in SYMBOLS)
    L = _capi.lib()
    # appended after ATTRIBUTE, nothing renumbered
    assert (_capi.UNSORTED, _capi.REFERENCE_CONFLICT) == (17, 18) and _capi.ATTRIBUTE == 16
    assert [L.bqsr_status_name(c).decode() for c in (16, 17, 18, 19)] == \
        ["ATTRIBUTE"] + _capi.MPILEUP_STATUS_NAMES + ["UNKNOWN"]
    assert _capi.BQSRError(17, "x").name == "UNSORTED" and _capi.BQSRError(18, "x").name == "REFERENCE_CONFLICT"
    with open(os.path.join(ROOT, "include", "adam_bqsr.h")) as fh:
        h = fh.read()
    assert "BQSR_ERR_UNSORTED = 17" in h and "BQSR_ERR_REFERENCE_CONFLICT = 18" in h
    # the sizes structure mirrors the header's, field for field
    with open(os.path.join(ROOT, "include", "adam_sam.h")) as fh:
        text = fh.read()
    body = text[text.index("typedef struct bqsr_mpileup_sizes {"):text.index("} bqsr_mpileup_sizes;")]
    fields = [l.split(";")[0].split()[-1] for l in body.splitlines()[1:] if ";" in l]
    assert fields == [f for f, _ in M.MpileupSizes._fields_] and ctypes.sizeof(M.MpileupSizes) == 32


def test_argument_checks_need_no_device():
    from adam_amd import mpileup as M
    L = M._lib()
    sz = M.MpileupSizes()
    n = ctypes.c_int64()
    assert L.bqsr_sam_mpileup_prepare(None, None, None, ctypes.byref(sz)) == _capi.INVALID_ARG
    assert L.bqsr_sam_mpileup_text(None, None, 0, 1, None, None, ctypes.byref(n), ctypes.byref(n)) == _capi.INVALID_ARG
    assert L.bqsr_arrow_mpileup_prepare(None, None, None, None, None, 0, None, 0, None,
                                        ctypes.byref(sz)) == _capi.INVALID_ARG
    assert L.bqsr_arrow_mpileup_text(None, None, 0, 1, None, None, ctypes.byref(n), ctypes.byref(n)) == _capi.INVALID_ARG
    assert L.bqsr_mpileup_kernel_times(None) == _capi.INVALID_ARG
    assert set(M.kernel_times()) == set(M.KERNELS)
