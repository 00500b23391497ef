#!/usr/bin/env python3
"""Correlation pass at the sizes a user runs: corr_sweep.py [repeats] > profiles/corr_sweep.txt

kcr_blocks_dev on one block of 2^22 lags (2^22 + K - 1 complex64 samples of uniform noise with a few copies of template 0
planted), for K in {64, 1024, 4096} x Q in {1, 8} (Q K <= 16384: K = 4096 runs Q = 1 and Q = 4), threshold 0.5 and guard K.
The call is the correlation kernel plus the peak stage (count, two scan kernels, emit), so the figure is what the caller waits
for.  One process, one GPU; after 3 warm-up launches every case is launched `repeats` times between two HIP events on the
object's stream and the median (min .. max) is reported.  The rate counts (8 Q + 4) K floating-point operations per lag, the
fused multiply-adds of the definition, against the 157.3 TFLOP/s of the fp32 vector pipes; beside it the least time the
samples, the dense outputs (none here) and the work buffers' traffic would take at 8 TB/s says which of the two binds."""
import importlib
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ksa = importlib.import_module("prgs-sdr-kspecanal_amd")

LAGS = 1 << 22
WARMUP = 3
PEAK_TF, VALU_GEMM_TF, HBM_TBS = 157.3, 52.0, 8.0
CASES = [(64, 1), (64, 8), (1024, 1), (1024, 8), (4096, 1), (4096, 4)]


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


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 11
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(20240601)
    print("# correlation pass: kcr_blocks_dev on one block of %d lags, complex64 samples, threshold 0.5, guard K, one MI355X," % LAGS)
    print("# median (min .. max) of %d launches between HIP events on the object's stream, after %d warm-up launches." % (repeats, WARMUP))
    print("# rate = (8 Q + 4) K operations per lag; yardsticks: %.1f TFLOP/s fp32 vector peak, %.0f TFLOP/s of the guide's VALU GEMM" % (
        PEAK_TF, VALU_GEMM_TF))
    print("# %5s %2s | %8s %8s %8s | %8s %7s %7s | %9s %6s | %6s | %s" % (
        "K", "Q", "ms med", "ms min", "ms max", "TFLOP/s", "of peak", "of GEMM", "ms at HBM", "binds", "events", "kernel_info"))
    for K, Q in CASES:
        n = LAGS + K - 1
        c = np.exp(2j * np.pi * rng.uniform(0, 1, (Q, K))).astype(np.complex64)
        x = (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)
        where = [1000 + i * (LAGS // 8) for i in range(8)]
        for s in where:
            x[s:s + K] += 4 * c[0]
        dev = torch.view_as_real(torch.from_numpy(x)).cuda()
        cr = ksa.Correlator(c, threshold=0.5, guard=K, capacity=4096, max_in=n, stream=stream.cuda_stream)
        t = timed(stream, lambda: cr.blocks_dev(dev, 1, n), repeats)
        ev, total = cr.events()
        assert total == len(where) * (repeats + WARMUP) and sorted(set(int(p) for p in ev["pos"])) == where, (K, Q, total)
        flops = (8 * Q + 4) * K * LAGS
        tf = flops / t[0] / 1e9
        # samples once, rho and r of every lag and template written once and rho read once by the peak stage
        hbm_ms = (8 * n + Q * LAGS * (4 + 8 + 4)) / (HBM_TBS * 1e12) * 1e3
        valu_ms = flops / (PEAK_TF * 1e12) * 1e3
        print("  %5d %2d | %8.3f %8.3f %8.3f | %8.2f %6.1f%% %6.1f%% | %9.3f %6s | %6d | %s" % (
            K, Q, t[0], t[1], t[2], tf, 100 * tf / PEAK_TF, 100 * tf / VALU_GEMM_TF, hbm_ms, "fp32" if valu_ms > hbm_ms else "HBM",
            total // (repeats + WARMUP), cr.kernel_info()))
        sys.stdout.flush()
        cr.close()
        del dev


if __name__ == "__main__":
    main()
