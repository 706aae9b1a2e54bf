"""`adam findreads` (adam-cli/.../cli/FindReads.scala:58-157): the joined
read buckets of two inputs whose comparison values meet a filter.

    python -m adam_amd.findreads INPUT1 INPUT2 FILTER [-file F] [-encoding1 E] [-encoding2 E]

FILTER is `;`-separated terms ``name(=|!=|<|>)value`` (compare.parse_filters);
a pair passes when every term is met by some value its comparison produced for
the pair.  The first output line is the combined comparison name, then one
line per passing pair: ``name \\t ref1:start1 \\t ref2:start2`` of each
bucket's first read in ReadBucket category order, rows ordered by bucket 1's
first read in input 1, then bucket 2's in input 2 (the reference's order is
Spark's collect()).  The join and the filter run on the device when one is
present (csrc/compare.hip), else in Python over SAM text.
"""
from __future__ import annotations

import argparse
import sys

from . import compare


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="adam_amd.findreads", description=__doc__.split("\n\n")[0])
    ap.add_argument("input1")
    ap.add_argument("input2")
    ap.add_argument("filter")
    ap.add_argument("-file", default=None, help="write the matching reads here instead of stdout")
    ap.add_argument("-encoding1", default="latin-1")
    ap.add_argument("-encoding2", default="latin-1")
    a = ap.parse_args(argv)
    name, rows = compare.find_reads(a.input1, a.input2, a.filter, a.encoding1, a.encoding2)
    text = compare.find_reads_text(name, rows)
    if a.file:
        with open(a.file, "w", encoding="latin-1") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
