"""The flagstat restatement (tests/_flagstat_ref.py) and the formatter, pinned
on a hand-written SAM whose counts are worked out below -- independently of
the device (tests/test_gpu_flagstat.py compares the device with the
restatement)."""
import pytest

from _adam_ref import convert_sam
from _flagstat_ref import NAMES, NullMapq, flagstat_ref, format_ref, java_2f_ref, percent_ref
from adam_amd.flagstat import FlagStatMetrics, format_flagstat, java_2f, percent

HEADER = b"@HD\tVN:1.4\n@SQ\tSN:chr1\tLN:1000000\n@SQ\tSN:chr2\tLN:1000000\n"


def line(name, flag, rname, mapq, rnext):
    pos = 0 if rname == "*" else 100
    pnext = 0 if rnext == "*" else 200
    return ("%s\t%d\t%s\t%d\t%d\t4M\t%s\t%d\t0\tACGT\tIIII\n" % (name, flag, rname, pos, mapq, rnext, pnext)).encode()


#         FLAG                                                   RNAME   MAPQ RNEXT
RECORDS = [
    ("r0", 0, "chr1", 60, "*"),        # FLAG 0: every boolean false (Q2) -- total only
    ("r1", 0x200 | 0x10, "chr1", 60, "*"),  # QC-failed, unpaired, mapped
    # primary duplicate, paired, proper, first, both mapped, mate on the same reference
    ("r2", 0x400 | 0x1 | 0x2 | 0x40, "chr1", 60, "="),
    # secondary duplicate, paired, second, mate unmapped: referenceId 0 != null -> cross chromosome
    ("r3", 0x400 | 0x100 | 0x1 | 0x80 | 0x8, "chr1", 30, "*"),
    # unpaired primary duplicate, RNAME set, RNEXT "*": mateMapped false (unpaired) -> only read
    # mapped; referenceId 1 != null -> cross chromosome (the duplicate counters ignore readPaired)
    ("r4", 0x400 | 0x10, "chr2", 60, "*"),
    ("r5", 0x1 | 0x8 | 0x40, "chr1", 60, "="),   # singleton, first
    ("r6", 0x1 | 0x4 | 0x80, "*", 0, "chr1"),    # read unmapped, mate mapped, second
    ("r7", 0x1 | 0x2 | 0x40, "chr1", 4, "chr2"),  # mate on another @SQ, MAPQ 4: diffChr, not MapQ5
    ("r8", 0x1 | 0x80, "chr1", 5, "chr2"),        # MAPQ 5: diffChr and MapQ5
    ("r9", 0x1 | 0x40 | 0x200, "chr2", 60, "chr1"),  # QC-failed; MAPQ 60: diffChr and MapQ5
    # RNAME not in @SQ: referenceId and mapq null; RNEXT "=" is then null too: null == null, not diffChr
    ("r10", 0x1 | 0x40, "chrUn", 60, "="),
    # secondary duplicate, both mapped, MAPQ 255 (mapq null) but "=": not diffChr, so mapq is never read
    ("r11", 0x1 | 0x80 | 0x400 | 0x100, "chr1", 255, "="),
]
SAM = HEADER + b"".join(line(*r) for r in RECORDS)

# passed: every record but r1 and r9
PASSED = (
    10,          # total
    2, 1, 1, 1,  # primary duplicates: r2 r4; both mapped: r2; only read mapped: r4; cross chromosome: r4
    2, 1, 1, 1,  # secondary duplicates: r3 r11; both mapped: r11; only read mapped: r3; cross chromosome: r3
    8,           # mapped: r2 r3 r4 r5 r7 r8 r10 r11 (r0: FLAG 0, r6: 0x4)
    8,           # paired: r2 r3 r5 r6 r7 r8 r10 r11
    4,           # read1: r2 r5 r7 r10
    4,           # read2: r3 r6 r8 r11
    2,           # properly paired: r2 r7
    5,           # with itself and mate mapped: r2 r7 r8 r10 r11
    2,           # singletons: r3 r5
    2,           # mate on a different chr: r7 r8
    1,           # ... with mapq >= 5: r8
)
FAILED = (
    2,           # r1 r9
    0, 0, 0, 0,
    0, 0, 0, 0,
    2,           # mapped: r1 r9
    1,           # paired: r9
    1,           # read1: r9
    0,
    0,
    1,           # with itself and mate mapped: r9
    0,
    1,           # mate on a different chr: r9
    1,           # MAPQ 60
)

TEXT = """
10 + 2 in total (QC-passed reads + QC-failed reads)
2 + 0 primary duplicates
1 + 0 primary duplicates - both read and mate mapped
1 + 0 primary duplicates - only read mapped
1 + 0 primary duplicates - cross chromosome
2 + 0 secondary duplicates
1 + 0 secondary duplicates - both read and mate mapped
1 + 0 secondary duplicates - only read mapped
1 + 0 secondary duplicates - cross chromosome
8 + 2 mapped (80.00%:100.00%)
8 + 1 paired in sequencing
4 + 1 read1
4 + 0 read2
2 + 0 properly paired (20.00%:0.00%)
5 + 1 with itself and mate mapped
2 + 0 singletons (20.00%:0.00%)
2 + 1 with mate mapped to a different chr
1 + 1 with mate mapped to a different chr (mapQ>=5)
""" + " " * 13


def test_hand_written_counts():
    failed, passed = flagstat_ref(convert_sam(SAM))
    assert dict(zip(NAMES, passed)) == dict(zip(NAMES, PASSED))
    assert dict(zip(NAMES, failed)) == dict(zip(NAMES, FAILED))


def test_null_mapq_throws():
    # diffChr with MAPQ 255 (r12), and with an RNAME outside @SQ against a resolved RNEXT (r13)
    text = SAM + line("r12", 0x1 | 0x40, "chr1", 255, "chr2") + line("r13", 0x1 | 0x40, "chrUn", 60, "chr2")
    with pytest.raises(NullMapq) as e:
        flagstat_ref(convert_sam(text))
    assert e.value.read == 12
    with pytest.raises(NullMapq) as e:
        flagstat_ref(convert_sam(SAM + line("r13", 0x1 | 0x40, "chrUn", 60, "chr2")))
    assert e.value.read == 12


@pytest.mark.parametrize("fmt, pct", [(java_2f_ref, percent_ref), (java_2f, percent)])
def test_percent_and_rounding(fmt, pct):
    assert fmt(pct(1, 800)) == "0.13"   # 0.125: half up on the shortest decimal (C's %.2f gives 0.12)
    assert "%.2f" % pct(1, 800) == "0.12"
    assert fmt(pct(0, 0)) == "0.00"
    assert fmt(pct(1, 8)) == "12.50"
    # the reference README's NA12878 figures
    total = 51554029
    assert fmt(pct(50849935, total)) == "98.63"
    assert fmt(pct(49874394, total)) == "96.74"
    assert fmt(pct(704094, total)) == "1.37"
    # the count passes through a 32-bit float: 2^24 + 1 is not one
    assert pct(16777217, 16777217) == 100.0 * 16777216.0 / 16777217


def test_text_literal():
    assert format_ref(FAILED, PASSED) == TEXT
    assert format_flagstat(FlagStatMetrics(*FAILED), FlagStatMetrics(*PASSED)) == TEXT
    assert TEXT.startswith("\n10 + 2") and TEXT.endswith("\n" + " " * 13) and TEXT.count("\n") == 19


def test_metrics_add():
    a, b = FlagStatMetrics(*PASSED), FlagStatMetrics(*FAILED)
    assert (a + b).counts() == tuple(x + y for x, y in zip(PASSED, FAILED))
    assert FlagStatMetrics().counts() == (0,) * 18
