"""A small seeded generator of SAM pairs for the `compare` tests: two inputs
that share most read names and differ the way two pipeline runs do (and in
the ways that exercise every branch of the join and the comparisons)."""
import random

HDR = b"@SQ\tSN:c\tLN:100000\n@SQ\tSN:d\tLN:100000\n@RG\tID:g\n@RG\tID:h\n"
# unpaired / first / second, primary and secondary (all mapped), then unmapped and FLAG 0
FLAGS = (16, 0x200, 0x41, 0x81, 0x61, 0x100, 0x141, 0x181, 4, 0x45, 0)
RGS = (b"g", b"h", None, b"nohdr")  # nohdr: an RG the header lacks reads as null


def rec(name, flag, qual, rg=b"g", ref=b"c", pos=10, mapq=60):
    n = 1 if qual == b"*" else len(qual)
    line = b"%s\t%d\t%s\t%d\t%d\t%dM\t*\t0\t0\t%s\t%s" % (name, flag, ref, pos, mapq, n, b"A" * n, qual)
    return line + (b"\tRG:Z:" + rg if rg is not None else b"") + b"\n"


def _qual(rng, n, wide):
    if wide and rng.random() < 0.05:
        return b"*"
    if wide and rng.random() < 0.15:  # bytes >= 0x80, and scores outside [0, 64): below '!' or above 'a'
        pool = list(range(0x80, 0x100)) + [0x20, 0x1F, 0x62, 0x7E, 0x7F]
        return bytes(rng.choice(pool) if rng.random() < 0.5 else rng.randrange(33, 97) for _ in range(n))
    return bytes(rng.randrange(33 + 2, 33 + 42) for _ in range(n))


def names(rng, n):
    """n distinct names of 1 to 254 bytes, most sharing long prefixes"""
    out, seen = [], set()
    stem = bytes(rng.randrange(48, 123) for _ in range(254)).replace(b"@", b"A")
    while len(out) < n:
        k = rng.choice((1, 2, 3, 8, 20, 40, 100, 200, 253, 254)) if rng.random() < 0.3 else rng.randrange(10, 60)
        nm = stem[:max(0, k - 3)] + b"%d" % rng.randrange(1000)
        nm = nm[:k] if len(nm) >= k else nm
        if nm and nm not in seen and not nm.startswith(b"@"):
            seen.add(nm)
            out.append(nm)
    return out


def gen_pair(seed, n_names, wide=True, long_pair=False, disjoint=False, mean_len=40):
    """(sam1, sam2) as bytes.  wide: quals with '*', bytes >= 0x80 and scores
    outside [0, 64) (side 2 is then latin-1 too); long_pair: one name whose
    reads hold 4096 bases on both sides; disjoint: no shared name."""
    rng = random.Random(seed)
    s1, s2 = [], []
    for nm in names(rng, n_names):
        reads = []
        for _ in range(rng.choice((1, 1, 1, 2, 2, 3, 4))):
            reads.append(dict(name=nm, flag=rng.choice(FLAGS) | (0x400 if rng.random() < 0.1 else 0),
                              rg=RGS[0] if rng.random() < 0.8 else rng.choice(RGS), ref=rng.choice((b"c", b"c", b"d")),
                              pos=rng.randrange(1, 90000), mapq=rng.randrange(0, 255),
                              qual=_qual(rng, max(1, int(rng.gauss(mean_len, 15))), wide)))
        if rng.random() < 0.05:  # the name in a second read group as well
            reads.append(dict(reads[0], rg=b"h" if reads[0]["rg"] != b"h" else b"g"))
        other = []
        for r in reads:
            r = dict(r)
            u = rng.random()
            if u < 0.05:
                continue                                   # the read is missing from side 2
            if u < 0.10 and r["flag"]:
                r["flag"] ^= 0x400                         # a duplicate on one side only
            elif u < 0.15:
                r["pos"] += rng.randrange(1, 50)           # a moved start
            elif u < 0.18:
                r["ref"] = b"d" if r["ref"] == b"c" else b"c"  # a moved reference
            elif u < 0.25:
                r["mapq"] = rng.randrange(0, 255)
            elif u < 0.45:
                r["qual"] = _qual(rng, max(1, len(r["qual"]) + rng.randrange(-3, 4)), wide)
            elif u < 0.75 and r["qual"] != b"*":
                q = bytearray(r["qual"])
                for _ in range(rng.randrange(1, 4)):
                    q[rng.randrange(len(q))] = rng.randrange(35, 75)
                r["qual"] = bytes(q)
            other.append(r)
            if rng.random() < 0.04:
                other.append(dict(r))                      # an overmatched category
        v = rng.random()
        if disjoint or v < 0.05:
            (s1 if rng.random() < 0.5 else s2).extend(reads)   # the whole name on one side only
        else:
            s1.extend(reads)
            s2.extend(other)
    if long_pair:
        q = bytes(rng.randrange(35, 75) for _ in range(4096))
        q2 = bytearray(q)
        for i in range(0, 4096, 97):
            q2[i] = 33 + rng.randrange(2, 42)
        s1.append(dict(name=b"long", flag=16, rg=b"g", ref=b"c", pos=5, mapq=60, qual=q))
        s2.append(dict(name=b"long", flag=16, rg=b"g", ref=b"c", pos=5, mapq=60, qual=bytes(q2)))
    rng.shuffle(s1)
    rng.shuffle(s2)
    return (HDR + b"".join(rec(**r) for r in s1), HDR + b"".join(rec(**r) for r in s2))


def fnv1a(data, h=0xcbf29ce484222325):
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def bucket_hash(rg_index, name):
    """the device's (recordGroupId, readName) key: rg_index None for no read group"""
    g = 0 if rg_index is None else rg_index + 1
    return fnv1a(name, fnv1a(g.to_bytes(4, "little")))
