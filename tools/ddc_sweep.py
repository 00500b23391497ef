#!/usr/bin/env python3
"""Down-converter rate over formats and shapes: ddc_sweep.py [repeats] > profiles/ddc_sweep.txt

kdc_process_dev (the stream form: the filter kernel and the history kernel) on 256 MiB of input per call, past the Infinity
Cache, for {c64, u8, s16} x (D, T) in {(4,32), (16,128), (16,256), (64,512), (256,2048)}, ddc_lowpass taps, the mixer on.  The
yardstick, taken in the same run and alternating with the kernel, is a device-to-device copy of the same input bytes (a
contiguous tensor copy: hipMemcpyAsync; it reads and writes those bytes).  One process, one GPU; after 2 warm-up rounds every
case is timed `repeats` times between two HIP events on the object's stream: median (min .. max).  Beside the rate: kernel time
over copy time, and the share of the larger of the two bounds of the arithmetic -- 4 T / D + 10 flop per input sample at
157.3 TFLOP/s fp32, and (sample bytes + 8 / D) bytes per input sample at 6.29 TB/s."""
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ksa = importlib.import_module("prgs-sdr-kspecanal_amd")

SHAPES = ((4, 32), (16, 128), (16, 256), (64, 512), (256, 2048))
FORMATS = (("c64", ksa.FMT_C64, 8), ("u8", ksa.FMT_U8, 2), ("s16", ksa.FMT_S16, 4))
INPUT_BYTES = 256 << 20
WARMUP = 2
PEAK_FLOPS, PEAK_BYTES = 157.3e12, 6.29e12
FORM = {0: "tile", 1: "reduce"}


def raw_input(fmt, n):
    g = torch.Generator(device="cuda").manual_seed(20201226)
    if fmt == ksa.FMT_C64:
        return torch.rand((n, 2), generator=g, device="cuda", dtype=torch.float32) * 2 - 1
    if fmt == ksa.FMT_U8:
        return torch.randint(0, 256, (2 * n,), generator=g, device="cuda", dtype=torch.uint8)
    return torch.randint(-32768, 32768, (2 * n,), generator=g, device="cuda", dtype=torch.int16)


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
    print("# down-converter: kdc_process_dev on %d MiB of input per call, one MI355X; median (min .. max) of %d calls between HIP"
          % (INPUT_BYTES >> 20, repeats))
    print("# events on the object's stream after %d warm-up rounds, alternating with a device-to-device copy of the same input bytes."
          % WARMUP)
    print("# bound: the larger of (4 T / D + 10) flop at %.1f TFLOP/s and (sample bytes + 8 / D) bytes at %.2f TB/s per input sample."
          % (PEAK_FLOPS / 1e12, PEAK_BYTES / 1e12))
    print("# %-4s %4s %5s | %8s %8s %8s | %8s | %8s %8s | %8s %-5s | %s" % (
        "fmt", "D", "T", "ms med", "ms min", "ms max", "GS/s in", "copy ms", "x copy", "of bound", "which", "kernel_info"))
    for name, fmt, nbytes in FORMATS:
        n = INPUT_BYTES // nbytes
        src = raw_input(fmt, n)
        dst = torch.empty_like(src)
        for D, T in SHAPES:
            dc = ksa.DownConverter(fmt, D, ksa.ddc_lowpass(D, T // D), freq=0.1234567, sampling_rate=1.0, max_in=n,
                                   stream=stream.cuda_stream)
            kern, copy = [], []
            with torch.cuda.stream(stream):
                for i in range(WARMUP + repeats):
                    c = once(stream, lambda: dst.copy_(src, non_blocking=True))
                    k = once(stream, lambda: dc.process_dev(src, n))
                    if i >= WARMUP:
                        copy.append(c)
                        kern.append(k)
            assert dc.state()["samples_in"] == n * (WARMUP + repeats)
            km, cm = spread(kern), spread(copy)
            t_flop = n * (4.0 * T / D + 10) / PEAK_FLOPS * 1e3
            t_byte = n * (nbytes + 8.0 / D) / PEAK_BYTES * 1e3
            print("  %-4s %4d %5d | %8.3f %8.3f %8.3f | %8.2f | %8.3f %8.2f | %7.1f%% %-5s | %s" % (
                name, D, T, km[0], km[1], km[2], n / km[0] / 1e6, cm[0], km[0] / cm[0], 100 * max(t_flop, t_byte) / km[0],
                "flop" if t_flop > t_byte else "HBM", {k: (FORM[v] if k == "form" else v) for k, v in dc.kernel_info().items()}))
            sys.stdout.flush()
            dc.close()
        del src, dst


if __name__ == "__main__":
    main()
