#!/usr/bin/env python3
"""The job tail in a `rocprofv3 --kernel-trace` of bench.py: per job (one
bqsr_observe_lean dispatch to the next) the gap from the observe kernel's end
to the apply kernel's start, apply's duration, and whether bqsr_fold_chain's
interval lies inside apply's (the speculative tail).

    python tools/tail_trace.py DIR [SKIP_JOBS]   (DIR searched for *kernel_trace.csv)
"""
import csv
import glob
import statistics
import sys


def main():
    d = sys.argv[1]
    skip = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    f = sorted(glob.glob(d + "/**/*kernel_trace.csv", recursive=True))[0]
    rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(open(f))]
    rows.sort(key=lambda r: r[1])
    jobs, cur = [], None
    for r in rows:
        if "bqsr_observe_lean" in r[0]:
            cur = [r]
            jobs.append(cur)
        elif cur is not None:
            cur.append(r)
    gaps, app, inside, chain_end_rel = [], [], [], []
    for j in jobs[skip:]:
        obs = j[0]
        ap = [r for r in j if r[0].startswith("bqsr_apply_kernel")]
        ch = [r for r in j if r[0].startswith("bqsr_fold_chain")]
        if not ap or not ch:
            continue
        gaps.append((ap[0][1] - obs[2]) / 1e3)
        app.append((ap[0][2] - ap[0][1]) / 1e3)
        inside.append(ap[0][1] <= ch[0][1] and ch[0][2] <= ap[0][2])
        chain_end_rel.append((ch[0][2] - ap[0][1]) / 1e3)
    print("%s: %d jobs" % (f, len(gaps)))
    print("  observe end -> apply start, us: median %.1f (min %.1f, max %.1f)" % (statistics.median(gaps), min(gaps), max(gaps)))
    print("  apply duration, us:             median %.1f (min %.1f, max %.1f)" % (statistics.median(app), min(app), max(app)))
    print("  bqsr_fold_chain inside apply's interval: %d of %d jobs; its end %.1f us (median) after apply's start"
          % (sum(inside), len(inside), statistics.median(chain_end_rel)))
    j = jobs[min(len(jobs) - 1, skip + 1)]
    t0 = j[0][1]
    print("  one job, us from the observe kernel's start: kernel, start, end")
    for r in j:
        print("    %-28s %9.1f %9.1f" % (r[0].split("(")[0][:28], (r[1] - t0) / 1e3, (r[2] - t0) / 1e3))


if __name__ == "__main__":
    main()
