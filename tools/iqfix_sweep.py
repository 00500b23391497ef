#!/usr/bin/env python3
"""IQ correction pass at the size a user runs: iqfix_sweep.py [repeats] > profiles/iqfix_sweep.txt

One kqf_blocks_dev / kqf_accumulate_dev call on one block of 2^24 samples (a tone plus noise through an impaired receiver) for
each sample format, in the three forms of the kernel: apply only, accumulate only and both.  One process, one GPU; after 3
warm-up launches every case is launched `repeats` times between two HIP events on the object's stream and the median
(min .. max) is reported: input GS/s, the bytes the pass moves (the sample bytes in, 8 bytes out per sample where it applies)
per second against the 8 TB/s HBM peak, and the least time that traffic would take at the peak.  The accumulating forms also
launch the finishing kernel, which is inside the timed span, and their sums are cleared outside it."""
import importlib
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ksa = importlib.import_module("prgs-sdr-kspecanal_amd")

N = 1 << 24
WARMUP = 3
HBM_TBS = 8.0
FORMATS = (("c64", 8), ("u8", 2), ("s8", 2), ("s16", 4))
FORMS = (("apply", True, False), ("accumulate", False, True), ("both", True, True))


def timed(stream, fn, between, repeats):
    for _ in range(WARMUP):
        fn()
        between()
    stream.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        between()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def samples(rng, fmt):
    """The capture in its format: a tone of 0.3 plus noise of 0.01, 1 dB and 5 degrees of imbalance, a DC offset."""
    t = np.arange(N)
    z = 0.3 * np.exp(2j * np.pi * 0.125 * t) + 0.01 * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    g, phi = 10 ** (1 / 20), np.radians(5.0)
    iq = np.stack([z.real + 0.05, g * (z.real * np.sin(phi) + z.imag * np.cos(phi)) - 0.03], axis=1)
    if fmt == "c64":
        return torch.from_numpy(iq.astype(np.float32)).cuda()
    if fmt == "u8":
        return torch.from_numpy(np.clip(np.rint(iq * 127.5 + 127.5), 0, 255).astype(np.uint8)).cuda()
    if fmt == "s8":
        return torch.from_numpy(np.rint(iq * 127).astype(np.int8)).cuda()
    return torch.from_numpy(np.rint(iq * 32767).astype(np.int16)).cuda()


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 11
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(20261020)
    print("# IQ correction pass: one call on one block of %d samples, the library's own output buffer, coefficients solved from the block," % N)
    print("# one MI355X, median (min .. max) of %d launches between HIP events on the object's stream, after %d warm-up launches." % (
        repeats, WARMUP))
    print("# TB/s = (sample bytes in + 8 bytes out where the form applies) / time; HBM peak %.1f TB/s; ms at HBM = that traffic at the peak" % HBM_TBS)
    print("# %4s %10s | %8s %8s %8s | %7s %6s %8s | %9s %7s | %s" % (
        "fmt", "form", "ms med", "ms min", "ms max", "GS/s", "TB/s", "of peak", "ms at HBM", "x HBM", "kernel_info"))
    for fmt, per in FORMATS:
        dev = samples(rng, fmt)
        fix = ksa.IqCorrector(fmt=fmt, max_in=N, stream=stream.cuda_stream)
        fix.accumulate_dev(dev, 1, N)
        sol = fix.solve("dc+iq")
        fix.clear_stats()
        for name, apply, acc in FORMS:
            if apply:
                fn = lambda: fix.blocks_dev(dev, 1, N, accumulate=acc)
            else:
                fn = lambda: fix.accumulate_dev(dev, 1, N)
            med, lo, hi = timed(stream, fn, fix.clear_stats if acc else (lambda: None), repeats)
            moved = N * (per + (8 if apply else 0))
            at_peak = moved / (HBM_TBS * 1e12) * 1e3
            print("  %4s %10s | %8.4f %8.4f %8.4f | %7.1f %6.3f %7.1f%% | %9.4f %7.2f | %s" % (
                fmt, name, med, lo, hi, N / med / 1e6, moved / med / 1e9, 100 * moved / med / 1e9 / HBM_TBS, at_peak, med / at_peak,
                fix.kernel_info()))
        print("#      %s solved to dc (%.6f, %.6f) c %.6f d %.6f flags %d" % (fmt, sol["dc_i"], sol["dc_q"], sol["c"], sol["d"], sol["flags"]))
        fix.close()
        del dev


if __name__ == "__main__":
    main()
