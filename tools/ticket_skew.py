#!/usr/bin/env python3
"""Finish-time spread of the persistent workgroups of one spectrum launch, from the records of a -DKSA_SKEW build
(KSA_SKEW_FILE=<file>: one line per workgroup and launch, "launch k wg xcc start end units", wall clock in 100 MHz ticks).

  tools/ticket_skew.py <file> [skip]      skip: launches at the head of the file that count as warm-up (default 3)

Per launch, over all workgroups and per XCD: first / median / last finish relative to the launch's first start, in us, and
(median - first), (last - median) as a percentage of the launch's duration (last finish - first start)."""
import sys
from collections import defaultdict
from statistics import median


def summarize(lines, skip=3):
    launches = defaultdict(list)
    for ln in lines:
        t = ln.split()
        if len(t) == 7 and t[0] == "launch":
            launches[int(t[1])].append(tuple(int(x) for x in t[2:]))   # wg, xcc, start, end, units
    out = []
    for k in sorted(launches)[skip:]:
        rec = launches[k]
        t0 = min(r[2] for r in rec)
        dur = max(r[3] for r in rec) - t0
        groups = [("all", rec)] + [("xcd%d" % x, [r for r in rec if r[1] == x]) for x in sorted({r[1] for r in rec})]
        out.append("launch %d: %d workgroups, %d units, duration %.1f us, last start %.1f us" %
                   (k, len(rec), sum(r[4] for r in rec), dur / 100.0, (max(r[2] for r in rec) - t0) / 100.0))
        for name, g in groups:
            fin = sorted(r[3] - t0 for r in g)
            first, med, last = fin[0], median(fin), fin[-1]
            units = sorted(r[4] for r in g)
            out.append("  %-5s wgs %4d  units/wg %3d..%3d  finish first %8.1f  median %8.1f  last %8.1f us   "
                       "median-first %5.2f %%  last-median %5.2f %%" %
                       (name, len(g), units[0], units[-1], first / 100.0, med / 100.0, last / 100.0,
                        100.0 * (med - first) / dur, 100.0 * (last - med) / dur))
    return out


if __name__ == "__main__":
    with open(sys.argv[1]) as f:
        print("\n".join(summarize(f.readlines(), int(sys.argv[2]) if len(sys.argv) > 2 else 3)))
