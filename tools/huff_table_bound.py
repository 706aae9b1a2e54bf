#!/usr/bin/env python3
"""The most second-level entries bgzf_inflate.hip's table_build needs over
every complete canonical Huffman code of at most N symbols and 15 bits, for
a root of R bits: python tools/huff_table_bound.py [N R] (default 30 8, the
distance code: 144 of kDistCap 256, over 4.3 million codes, half a minute).
The 286-symbol literal/length code is out of this enumeration's reach; its
bound is zlib's (enough.c: 852 entries in all at root 9, 340 of kLitCap 512
in the second level)."""
import sys


def entries(counts, root):
    """table_build's `off` for a code with counts[l - 1] codes of l bits."""
    code, off, gprev, gbits = 0, 0, -1, 0
    for l, c in enumerate(counts, 1):
        if l > root:
            for j in range(c):
                g = (code + j) >> (l - root)
                if g != gprev:
                    if gprev >= 0:
                        off += 1 << gbits
                    gprev = g
                gbits = l - root
        code = (code + c) << 1
    return off + ((1 << gbits) if gprev >= 0 else 0)


def bound(n_sym, root):
    best, n = [0, None], [0]

    def rec(l, left, syms, counts):  # left: unassigned codes of l bits; every one takes at least a symbol
        for c in range(min(left, syms) + 1):
            if left == c:
                n[0] += 1
                e = entries(counts + [c], root)
                if e > best[0]:
                    best[:] = [e, counts + [c]]
            elif l < 15 and 2 * (left - c) <= syms - c:
                rec(l + 1, 2 * (left - c), syms - c, counts + [c])

    rec(1, 2, n_sym, [])
    return best[0], best[1], n[0]


if __name__ == "__main__":
    n_sym, root = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (30, 8)
    e, counts, n = bound(n_sym, root)
    print("%d symbols, root %d: at most %d second-level entries (codes per length %s), %d codes" % (n_sym, root, e, counts, n))
