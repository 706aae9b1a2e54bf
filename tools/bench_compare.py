"""`compare` throughput: a synthetic SAM (samgen) against its own
`transform -mark_duplicate_reads -recalibrate_base_qualities` SAM output, all
five comparisons, side 2 read as UTF-8; prints one JSON line.

  reads/s end to end (both files read, parsed, compared on the device), the
  device-event times of the join, scalar and baseqs kernels, the baseqs pass
  as bytes of qual read per second next to a device-to-device copy rate
  measured in the same run, and the baseline: compare.compare_baseqs (the
  single-threaded Python path, one comparison) on the first --baseline-reads
  reads of the same pair, both as seconds per million reads."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def head(path, out, n_reads):
    """the header and the first n_reads records"""
    k = 0
    with open(path, "rb") as src, open(out, "wb") as dst:
        for line in src:
            if not line.startswith(b"@"):
                if k == n_reads:
                    break
                k += 1
            dst.write(line)


def copy_rate_gbs(torch, n_bytes=1 << 30, reps=5):
    """bytes read + written per second of a device-to-device copy"""
    a = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    b.copy_(a)
    best = None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    return 2.0 * n_bytes / (best * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--baseline-reads", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    from adam_amd import compare, synth
    from adam_amd.samgen import sam_text
    from adam_amd.transform import transform
    torch.zeros(1, device="cuda")
    with tempfile.TemporaryDirectory() as d:
        p1, p2 = os.path.join(d, "in.sam"), os.path.join(d, "out.sam")
        t0 = time.perf_counter()
        b = synth.generate(a.reads, (100,), 2, 20261019, contig_len=max(1000, a.reads * 100 // 30))
        with open(p1, "wb") as fh:
            fh.write(sam_text(b, n_rg=2, qname="q"))
        transform(p1, p2, mark_duplicates=True, recalibrate=True)
        t_gen = time.perf_counter() - t0
        times, kernel, r = [], (0.0, 0.0, 0.0), None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = compare.compare_device(p1, p2, "all", "latin-1", "utf-8")
            t = time.perf_counter() - t0
            if not times or t < min(times):
                kernel = r.stats["kernel_ms"]
            times.append(t)
        t = min(times)
        n = a.reads
        h1, h2 = os.path.join(d, "h1.sam"), os.path.join(d, "h2.sam")
        nb = min(a.baseline_reads, n)
        head(p1, h1, nb)
        head(p2, h2, nb)
        t0 = time.perf_counter()
        base = compare.compare_baseqs(h1, h2, "latin-1", "utf-8")
        t_base = time.perf_counter() - t0
        hb = compare.compare_device(h1, h2, ["baseqs"], "latin-1", "utf-8")
        assert hb.histograms["baseqs"] == dict(base["histogram"]), "device and baseline disagree"
        chars = int(r.stats["baseq_chars"])
        out = {
            "metric": "compare (5 comparisons) reads/s end to end, two SAM files of --reads reads each",
            "reads_per_side": n, "seconds": t, "reads_per_s": 2 * n / t,
            "seconds_per_million_reads": t / (n / 1e6),
            "joined_pairs": int(r.stats["pairs"]), "baseq_chars": chars,
            "kernel_ms": {"join": kernel[0], "scalar": kernel[1], "baseqs": kernel[2]},
            "baseqs_qual_gbs": 2.0 * chars / (kernel[2] * 1e-3) / 1e9 if kernel[2] else None,
            "device_copy_gbs": copy_rate_gbs(torch),
            "baseline": {"what": "compare_baseqs (host Python, baseqs only)", "reads_per_side": nb, "seconds": t_base,
                         "seconds_per_million_reads": t_base / (nb / 1e6)},
            "summary": {c: [compare.hist_count(h), compare.hist_identical(h)] for c, h in r.histograms.items()},
            "gen_seconds": t_gen,
        }
        print(json.dumps(out))


if __name__ == "__main__":
    main()
