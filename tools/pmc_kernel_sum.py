#!/usr/bin/env python3
"""Per-launch averages of every counter collected in the passes under a profile directory
(rocprofv3 --pmc ... -d <dir>/<pass> -o run --output-format csv), for the kernels whose name
contains a pattern.  usage: tools/pmc_kernel_sum.py [--per-xcc] <dir> [pattern ...]

--per-xcc: the counters named <NAME>_xcc<k> (tools/profile_bench.sh's xtcc / xsq passes: one
derived counter per XCC, since the CSV sums a counter's dimensions) as one row per counter and
one column per XCC, with the mean, the largest and largest / mean; TCC_HIT and TCC_MISS also
give the hit rate per XCC."""
import collections
import csv
import glob
import os
import re
import sys


def collect(root, pat):
    acc = collections.defaultdict(float)
    n = collections.defaultdict(set)
    for f in sorted(glob.glob(os.path.join(root, "*", "run_counter_collection.csv"))):
        for r in csv.DictReader(open(f)):
            if pat not in r["Kernel_Name"]:
                continue
            c = r["Counter_Name"]
            acc[c] += float(r["Counter_Value"])
            n[c].add(r["Dispatch_Id"])
    return {c: acc[c] / max(1, len(n[c])) for c in acc}, {c: len(n[c]) for c in acc}


def per_xcc(avg, launches):
    rows = collections.defaultdict(dict)
    for c, v in avg.items():
        m = re.fullmatch(r"(.+)_xcc(\d+)", c)
        if m:
            rows[m.group(1)][int(m.group(2))] = v
    if not rows:
        print("  (no <NAME>_xcc<k> counters: run the xtcc / xsq passes)")
        return
    nx = 1 + max(k for r in rows.values() for k in r)
    print("  " + " " * 22 + "".join(f"{'xcc' + str(k):>12s}" for k in range(nx)) +
          f"{'mean':>12s}{'max':>12s}{'max/mean':>10s}")

    def line(name, v, fmt):
        mean = sum(v) / len(v)
        print(f"  {name:22s}" + "".join(f"{x:12{fmt}}" for x in v) +
              f"{mean:12{fmt}}{max(v):12{fmt}}{max(v) / mean if mean else 0.0:10.3f}")

    for name in sorted(rows):
        line(name, [rows[name].get(k, 0.0) for k in range(nx)], ".0f")
    if "TCC_HIT" in rows and "TCC_MISS" in rows:
        h, m = rows["TCC_HIT"], rows["TCC_MISS"]
        line("hit rate", [h.get(k, 0.0) / max(1.0, h.get(k, 0.0) + m.get(k, 0.0))
                          for k in range(nx)], ".4f")
    print(f"  ({max(launches.values())} launches)")


def main():
    argv = sys.argv[1:]
    xcc = "--per-xcc" in argv
    argv = [a for a in argv if a != "--per-xcc"]
    root = argv[0]
    pats = argv[1:] or ["k_h_eval"]
    for pat in pats:
        avg, launches = collect(root, pat)
        print(f"== {pat}")
        if xcc:
            per_xcc(avg, launches)
            continue
        for c in sorted(avg):
            print(f"  {c:40s} {avg[c]:16.1f}  ({launches[c]} launches)")


if __name__ == "__main__":
    main()
