"""The -sort_reads restatement (tests/_sort_ref.py) pinned: the reference's
own suite, hand-written orders, the unmapped counter's wrap, and the six
reference fixtures.  No GPU."""
import os

import pytest

from _sort_ref import (INT_MAX, LONG_MAX, sam_keys, sort_keys_ref, sort_order_ref, sorted_sam, split_sam,
                       suite_reads)
from adam_amd.records import read_sam_records

GOLD = os.path.join(os.path.dirname(__file__), "golden", "reference_resources")


def test_reference_suite_sorting_reads():
    mapped, ref, start = suite_reads()
    order = sort_order_ref(mapped, ref, start)
    assert sorted(order) == list(range(1000))
    where_mapped = [k for k, i in enumerate(order) if mapped[i]]
    where_unmapped = [k for k, i in enumerate(order) if not mapped[i]]
    assert where_mapped and where_unmapped
    # every unmapped read is placed behind the last mapped one
    assert min(where_unmapped) > max(where_mapped)
    # the mapped reads are sorted by (referenceId, start)
    keys = [(ref[i], start[i]) for i in order if mapped[i]]
    assert all(a <= b for a, b in zip(keys, keys[1:]))


def test_five_reads_by_hand():
    #          0: chr1:50  1: 0x4     2: chr0:99  3: chr1:50  4: FLAG 0 with coordinates (Q2: not mapped)
    mapped = [True, False, True, True, False]
    ref = [1, None, 0, 1, 1]
    start = [50, None, 99, 50, 7]
    assert sort_keys_ref(mapped, ref, start) == [(1, 50), (INT_MAX - 1, LONG_MAX), (0, 99), (1, 50),
                                                 (INT_MAX - 2, LONG_MAX)]
    # the tie 0 / 3 keeps its input order; the unmapped reads come in reverse
    assert sort_order_ref(mapped, ref, start) == [2, 0, 3, 4, 1]


def test_unmapped_counter_wraps():
    n = 10002
    order = sort_order_ref([False] * n, [None] * n, [None] * n)
    # 1-based ordinals: 10000, 9999, .., 2, 1, 10002, 10001
    assert [i + 1 for i in order] == list(range(10000, 0, -1)) + [10002, 10001]


def test_mapped_read_with_null_field_raises():
    with pytest.raises(TypeError):
        sort_order_ref([True], [None], [5])
    with pytest.raises(TypeError):
        sort_order_ref([False, True], [None, 3], [None, None])
    assert sort_order_ref([False], [None], [None]) == [0]


@pytest.mark.parametrize("name, moved", [("artificial.realigned.sam", 0), ("artificial.sam", 0),
                                         ("small_realignment_targets.sam", 0), ("reads12.sam", 198),
                                         ("small.sam", 18), ("unmapped.sam", 198)])
def test_reference_fixtures(name, moved):
    path = os.path.join(GOLD, name)
    text = open(path, "rb").read()
    mapped, ref, start = sam_keys(text)
    # the helper's keys are those of the converter's records
    recs = read_sam_records(path)
    assert mapped == [bool(r.read_mapped) for r in recs]
    assert start == [r.start for r in recs]
    assert [r is None for r in ref] == [r.reference_name is None for r in recs]
    # no mapped read with a null field
    order = sort_order_ref(mapped, ref, start)
    assert sum(1 for k, i in enumerate(order) if k != i) == moved
    header, lines = split_sam(text)
    if moved == 0:
        assert sorted_sam(text) == header + b"".join(l + b"\n" for l in lines)
