#!/usr/bin/env python3
"""Pulse detection pass at the sizes a user runs: pulse_sweep.py [repeats] > profiles/pulse_sweep.txt

kpl_blocks_dev on one block of 2^24 samples (weak noise with 64 planted bursts of 10 000 samples) for each sample format at
W in {1, 16, 256, 4096}, no dense output, min_len 16.  The call is the five launches of the block form (envelope, states, runs,
stitch, records), so the figure is what the caller waits for.  One process, one GPU; after 3 warm-up launches every case is
launched `repeats` times between two HIP events on the object's stream and the median (min .. max) is reported: input GS/s, and
the input bytes per second against the 8 TB/s HBM peak.  The input is read twice (envelope and runs) and, at large W, the halo
of W - 1 samples once more per tile of 2048, and S is written and read once at 8 bytes per sample: the last column is the least
time that traffic would take at the peak."""
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
BURSTS, BURST_LEN = 64, 10000
FORMATS = (("c64", 8), ("u8", 2), ("s8", 2), ("s16", 4))
WINDOWS = (1, 16, 256, 4096)


def timed(stream, fn, repeats):
    for _ in range(WARMUP):
        fn()
    stream.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def samples(rng, fmt):
    """The capture in its format: amplitude 0.01 noise, 0.5 inside the bursts."""
    amp = np.full(N, 0.01)
    for i in range(BURSTS):
        s = 5000 + i * (N // BURSTS)
        amp[s:s + BURST_LEN] = 0.5
    z = amp * np.exp(2j * np.pi * rng.uniform(0, 1, N))
    if fmt == "c64":
        return torch.view_as_real(torch.from_numpy(z.astype(np.complex64))).cuda()
    iq = np.stack([z.real, z.imag], axis=1)
    if fmt == "u8":
        return torch.from_numpy(np.clip(np.rint(iq * 127.5 + 127.5), 0, 255).astype(np.uint8)).cuda()
    if fmt == "s8":
        return torch.from_numpy(np.rint(iq * 127).astype(np.int8)).cuda()
    return torch.from_numpy(np.rint(iq * 32767).astype(np.int16)).cuda()


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 11
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(20240901)
    print("# pulse detection pass: kpl_blocks_dev on one block of %d samples, %d bursts of %d samples, on 0.05 off 0.02, min_len 16," % (
        N, BURSTS, BURST_LEN))
    print("# one MI355X, median (min .. max) of %d launches between HIP events on the object's stream, after %d warm-up launches." % (
        repeats, WARMUP))
    print("# input TB/s = sample bytes / time; HBM peak %.1f TB/s; ms at HBM = (2 x input + halo + 16 bytes of S per sample) at the peak" % HBM_TBS)
    print("# %4s %5s | %8s %8s %8s | %7s %10s %8s | %9s | %6s | %s" % (
        "fmt", "W", "ms med", "ms min", "ms max", "GS/s", "input TB/s", "of peak", "ms at HBM", "pulses", "kernel_info"))
    for fmt, per in FORMATS:
        dev = samples(rng, fmt)
        for W in WINDOWS:
            det = ksa.PulseDetector(W=W, on_power=0.05, off_power=0.02, min_len=16, capacity=4096, max_in=N, fmt=fmt,
                                    stream=stream.cuda_stream)
            t = timed(stream, lambda: det.blocks_dev(dev, 1, N), repeats)
            ev, total, active = det.events()
            assert total == BURSTS * (repeats + WARMUP), (fmt, W, total)
            tile = det.kernel_info()["tile"]
            gs = N / t[0] / 1e6
            tbs = N * per / t[0] / 1e9
            hbm_ms = (N * per * (2 + (W - 1) / tile) + 16 * N) / (HBM_TBS * 1e12) * 1e3
            print("  %4s %5d | %8.3f %8.3f %8.3f | %7.2f %10.3f %7.1f%% | %9.3f | %6d | %s" % (
                fmt, W, t[0], t[1], t[2], gs, tbs, 100 * tbs / HBM_TBS, hbm_ms, total // (repeats + WARMUP), det.kernel_info()))
            sys.stdout.flush()
            det.close()
        del dev


if __name__ == "__main__":
    main()
