#!/usr/bin/env python3
"""PSD fold against the AVG fold, spectrum stage only (tools/bench_one.py run()): psd_sweep.py [repeats] > profiles/psd_sweep.txt

One process, one GPU; per shape the AVG and the PSD engine alternate `repeats` times.  AVG's kernels are the baseline.  The
two folds segment a block differently when the hop is fractional (K:386 against matplotlib's constant step), so they are
compared per window: ns per window and frame.  Bar: PSD's median is not above AVG's by more than the spread (max - min) of
AVG's own repeats."""
import statistics
import sys

from bench_one import run

SHAPES = [  # name, N, nonOverlap, window, fullSize, frames
    ("C2 4096 / 0.5 / hanning", 4096, 0.5, "hanning", 32768, 16384),
    ("C3 16384 kaiser", 16384, 0.1, "kaiser", 131072, 2304),
    ("C4 64, 71 windows", 64, 0.1, "ones", 512, 1226 * 64),
    ("C5 65536, 75 % overlap", 65536, 0.25, "hanning", 524288, 256),
    ("1024 pair-sized batch", 1024, 0.5, "hanning", 8192, 65536),
    ("2400 mixed radix", 2400, 0.5, "hanning", 19200, 4096),
]


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    print("# PSD fold against AVG fold: spectrum-stage time (ksa_prof_read, mean of 5 launches per run), complex64, dB output,")
    print("# one MI355X, AVG and PSD engines alternating %d times per shape.  ns = time per window and frame." % repeats)
    print("# %-26s %5s %9s %9s | %8s %8s %8s | %8s %8s | %7s %s" % ("shape", "fold", "windows", "vgprs", "ns min", "ns med", "ns max",
                                                                     "ms med", "MFFT/s", "PSD/AVG", "verdict"))
    for name, n, q, win, full, frames in SHAPES:
        ns = {"AVG": [], "PSD": []}
        meta = {}
        for _ in range(repeats):
            for fold in ("AVG", "PSD"):
                ms, nwin, vgprs = run(n, q, win, full, frames, fold)
                ns[fold].append(ms * 1e6 / (nwin * frames))
                meta[fold] = (nwin, vgprs, ms)
        med = {f: statistics.median(v) for f, v in ns.items()}
        spread = max(ns["AVG"]) - min(ns["AVG"])
        verdict = "ok" if med["PSD"] <= med["AVG"] + spread else "SLOWER than AVG + its spread"
        for fold in ("AVG", "PSD"):
            nwin, vgprs, _ = meta[fold]
            tail = "| %7.3f %s" % (med["PSD"] / med["AVG"], verdict) if fold == "PSD" else "| (spread %.3f ns)" % spread
            print("  %-26s %5s %9d %9d | %8.3f %8.3f %8.3f | %8.3f %8.2f %s" % (
                name, fold, nwin, vgprs, min(ns[fold]), med[fold], max(ns[fold]), med[fold] * nwin * frames / 1e6,
                1e3 / med[fold], tail))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
