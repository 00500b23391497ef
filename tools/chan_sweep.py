#!/usr/bin/env python3
"""Channelizer rate over formats and shapes: chan_sweep.py [repeats] > profiles/chan_sweep.txt

kch_process_dev (the stream form: the channelizer kernel and the history kernel) on 2^26 input samples per call, input and
output both past the Infinity Cache, for {c64, u8, s16} x (M, O, P) below, chan_prototype taps.  In the same run, alternating
with it: one kdc_process_dev call of the same D, T and format (one channel by the down-converter; all M channels cost about one
such call plus the transform and the M / D times larger write), and at O = 1 and c64 the engine's KSA_CUMU_PFB path at
fft_size = M, pfbTaps = P over the same samples with frames M apart (the nearest existing kernel doing the same filter and
transform; it writes a dB row instead of the complex result).  One process, one GPU; after 2 warm-up rounds every case is timed
`repeats` times between two HIP events on the object's stream: median (min .. max).  Beside the rate: the achieved share of
6.29 TB/s on the algorithmic bytes, sample bytes + 8 O per input sample, and the share of the arithmetic bound,
4 T / D + 5 O log2 M flop per input sample at 157.3 TFLOP/s."""
import importlib
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ksa = importlib.import_module("prgs-sdr-kspecanal_amd")

SHAPES = ((16, 1, 8), (64, 1, 8), (64, 2, 8), (256, 1, 8), (256, 2, 8), (256, 4, 8), (1024, 1, 8), (1024, 4, 8))
FORMATS = (("c64", ksa.FMT_C64, 8), ("u8", ksa.FMT_U8, 2), ("s16", ksa.FMT_S16, 4))
SAMPLES = 1 << 26
WARMUP = 2
PEAK_FLOPS, PEAK_BYTES = 157.3e12, 6.29e12


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
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 11
    stream = torch.cuda.Stream()
    n = SAMPLES
    print("# channelizer: kch_process_dev on 2^%d input samples per call, one MI355X; median (min .. max) of %d calls between HIP"
          % (int(math.log2(n)), repeats))
    print("# events on the object's stream after %d warm-up rounds, alternating with one kdc_process_dev call of the same D, T and format"
          % WARMUP)
    print("# (and, at O = 1 and c64, the engine's KSA_CUMU_PFB path at fft_size M, pfbTaps P, frames M apart).")
    print("# of HBM: (sample bytes + 8 O) bytes per input sample over the time, against %.2f TB/s; of flop: 4 T / D + 5 O log2 M flop per"
          % (PEAK_BYTES / 1e12))
    print("# input sample against %.1f TFLOP/s." % (PEAK_FLOPS / 1e12))
    print("# %-4s %5s %2s %3s | %8s %8s %8s | %8s | %7s %7s | %8s %7s | %8s | %s" % (
        "fmt", "M", "O", "P", "ms med", "ms min", "ms max", "GS/s in", "of HBM", "of flop", "ddc ms", "x ddc", "pfb ms", "kernel_info"))
    for name, fmt, nbytes in FORMATS:
        src = raw_input(fmt, n)
        for M, O, P in SHAPES:
            D, T = M // O, M * P
            taps = ksa.chan_prototype(M, P)
            ch = ksa.Channelizer(fmt, M, O, taps, max_in=n, stream=stream.cuda_stream)
            dc = ksa.DownConverter(fmt, D, taps, phase_inc=2 ** 64 // M, max_in=n, stream=stream.cuda_stream)
            eng, pfb, nframes = None, [], n // M - P + 1
            if O == 1 and fmt == ksa.FMT_C64:
                try:
                    eng = ksa.SpectrumEngine(M, pfb_taps=P, window="hamming", max_frames=nframes, stream=stream.cuda_stream)
                except ksa.KsaError as e:
                    print("# pfb M %d P %d refused: %s" % (M, P, e))
            kern, ddc = [], []
            with torch.cuda.stream(stream):
                for i in range(WARMUP + repeats):
                    k = once(stream, lambda: ch.process_dev(src, n))
                    c = once(stream, lambda: dc.process_dev(src, n))
                    f = once(stream, lambda: eng.frames_dev(src, fmt, nframes, frame_stride=M)) if eng is not None else None
                    if i >= WARMUP:
                        kern.append(k)
                        ddc.append(c)
                        if f is not None:
                            pfb.append(f)
            assert ch.state()["samples_in"] == n * (WARMUP + repeats)
            km, dm = spread(kern), spread(ddc)
            t_flop = n * (4.0 * T / D + 5.0 * O * math.log2(M)) / PEAK_FLOPS * 1e3
            t_byte = n * (nbytes + 8.0 * O) / PEAK_BYTES * 1e3
            print("  %-4s %5d %2d %3d | %8.3f %8.3f %8.3f | %8.2f | %6.1f%% %6.1f%% | %8.3f %7.2f | %8s | %s" % (
                name, M, O, P, km[0], km[1], km[2], n / km[0] / 1e6, 100 * t_byte / km[0], 100 * t_flop / km[0], dm[0], km[0] / dm[0],
                "%.3f" % spread(pfb)[0] if pfb else "-", ch.kernel_info()))
            sys.stdout.flush()
            ch.close()
            dc.close()
            if eng is not None:
                eng.close()
        del src


if __name__ == "__main__":
    main()
