#!/usr/bin/env python3
"""Demodulator rate over shapes and variants: demod_sweep.py [N] > profiles/demod_sweep.txt

kdm_process_dev (the stream form: the filter kernel and the history kernel) on 2^26 complex64 samples (512 MiB, past the
Infinity Cache) per call: FM with float32 output at (D, T) in {(1,33), (5,80), (16,128), (64,1024)}, and the AM and the int16
variants at (5,80); demod_taps where T is a whole number of phases, else the same formula at that T.  Two yardsticks are taken
in the same run, alternating with the kernel: kdc_process_dev of libksa_ddc with the same D, T, input and phase_inc 0, and a
device-to-device copy of the input (a contiguous tensor copy: it reads and writes those bytes).  One process, one GPU; after 3
warm-up rounds every case is timed N times between two HIP events on the object's stream: median (min .. max).  Beside the
rate: kernel time over copy time and over down-converter time, and which of the three bounds of the per-sample arithmetic is
the largest -- T / D fused multiply-adds plus the detector's instructions (AM 17, PM 46, FM 55: history_kernel's listing less its 20 of indexing) at
78.6 T lane-instructions/s, 8 + 4 / D bytes at 6.29 TB/s of HBM, and 4 T / D + 4 bytes at 75 TB/s of ds_read_b32."""
import importlib
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ksa = importlib.import_module("prgs-sdr-kspecanal_amd")

CASES = (("fm", "f32", 1, 33), ("fm", "f32", 5, 80), ("fm", "f32", 16, 128), ("fm", "f32", 64, 1024),
         ("am", "f32", 5, 80), ("fm", "s16", 5, 80))
N_IN = 1 << 26
WARMUP = 3
PEAK_VALU, PEAK_HBM, PEAK_LDS = 78.6e12, 6.29e12, 75e12
DETECTOR = {"am": 17, "pm": 46, "fm": 55}


def taps_for(D, T):
    if T % D == 0:
        return ksa.demod_taps(D, T // D)
    t = np.arange(T, dtype=np.float64) - (T - 1) / 2
    h = np.sinc(0.8 * t / D) * np.hamming(T)
    return (h / h.sum()).astype(np.float32)


def once(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def spread(ms):
    return statistics.median(ms), min(ms), max(ms)


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    stream = torch.cuda.Stream()
    print("# demodulator: kdm_process_dev on 2^26 complex64 samples (512 MiB) per call, one MI355X; median (min .. max) of %d calls"
          % repeats)
    print("# between HIP events on the object's stream after %d warm-up rounds, alternating with kdc_process_dev (same D, T, input,"
          % WARMUP)
    print("# phase_inc 0) and a device-to-device copy of the input.  bound: the largest of (T / D + detector) lane-instructions at")
    print("# %.1f T/s, (8 + 4 / D) bytes at %.2f TB/s of HBM and (4 T / D + 4) bytes at %.0f TB/s of LDS, per input sample."
          % (PEAK_VALU / 1e12, PEAK_HBM / 1e12, PEAK_LDS / 1e12))
    print("# %-4s %-4s %4s %5s | %8s %8s %8s | %8s | %8s %7s | %8s %7s | %8s %-5s | %s" % (
        "mode", "out", "D", "T", "ms med", "ms min", "ms max", "GS/s in", "copy ms", "x copy", "ddc ms", "x ddc", "of bound", "which",
        "kernel_info"))
    g = torch.Generator(device="cuda").manual_seed(20201226)
    src = torch.rand((N_IN, 2), generator=g, device="cuda", dtype=torch.float32) * 2 - 1
    dst = torch.empty_like(src)
    for mode, out_fmt, D, T in CASES:
        taps = taps_for(D, T)
        dm = ksa.Demodulator(mode, D, taps, out_fmt=out_fmt, max_in=N_IN, stream=stream.cuda_stream)
        dc = ksa.DownConverter(ksa.FMT_C64, D, taps, phase_inc=0, max_in=N_IN, stream=stream.cuda_stream)
        kern, conv, copy = [], [], []
        with torch.cuda.stream(stream):
            for i in range(WARMUP + repeats):
                c = once(stream, lambda: dst.copy_(src, non_blocking=True))
                v = once(stream, lambda: dc.process_dev(src, N_IN))
                k = once(stream, lambda: dm.process_dev(src, N_IN))
                if i >= WARMUP:
                    copy.append(c)
                    conv.append(v)
                    kern.append(k)
        assert dm.state()["samples_in"] == N_IN * (WARMUP + repeats)
        km, vm, cm = spread(kern), spread(conv), spread(copy)
        bounds = {"VALU": N_IN * (T / D + DETECTOR[mode]) / PEAK_VALU * 1e3, "HBM": N_IN * (8 + 4.0 / D) / PEAK_HBM * 1e3,
                  "LDS": N_IN * (4.0 * T / D + 4) / PEAK_LDS * 1e3}
        which = max(bounds, key=bounds.get)
        print("  %-4s %-4s %4d %5d | %8.3f %8.3f %8.3f | %8.2f | %8.3f %7.2f | %8.3f %7.2f | %7.1f%% %-5s | %s" % (
            mode, out_fmt, D, T, km[0], km[1], km[2], N_IN / km[0] / 1e6, cm[0], km[0] / cm[0], vm[0], km[0] / vm[0],
            100 * bounds[which] / km[0], which, dm.kernel_info()))
        sys.stdout.flush()
        dm.close()
        dc.close()


if __name__ == "__main__":
    main()
