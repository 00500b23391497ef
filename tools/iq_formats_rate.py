#!/usr/bin/env python3
"""Rates of the four sample formats: iq_formats_rate.py [repeats] > profiles/iq_formats.txt

Part 1, device-resident, config 2 shape (fftSize 4096, 50 % overlap, hanning, 16384 blocks of 32768 samples): spectrum-stage
time (ksa_prof_read, mean of 5 launches per run) of complex64, uint8, int8 and int16 input, the four engines alternating
`repeats` times in one process.  M FFT/s = windows transformed per microsecond.  The comparison is against the complex64 and
uint8 figures of this same run; a format whose median is below complex64's by more than the spread (max - min) of complex64's
own repeats is marked.

Part 2, page-locked host memory as the IQ pointer (ksa_frames_dev reading a PinnedBuffer over the host link: the route of
int8 / int16 numpy blocks) next to ksa_frames_u8 from the same kind of memory, wall time around call + synchronise,
alternating `repeats` times.  GS/s = samples per nanosecond."""
import importlib
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ksa = importlib.import_module("prgs-sdr-kspecanal_amd")

N, Q, WIN, FULL, FRAMES = 4096, 0.5, "hanning", 32768, 16384
FORMATS = (("c64", ksa.FMT_C64), ("u8", ksa.FMT_U8), ("s8", ksa.FMT_S8), ("s16", ksa.FMT_S16))


def device_blocks(name, frames):
    """[frames][...] on the device: 64 MiB of distinct random blocks, tiled."""
    rng = np.random.default_rng(7)
    distinct = min(frames, 256)
    if name == "c64":
        host = torch.from_numpy(rng.standard_normal((distinct, 2 * FULL), dtype=np.float32) * np.float32(0.3))
    elif name == "u8":
        host = torch.from_numpy(rng.integers(0, 256, (distinct, 2 * FULL), dtype=np.uint8))
    elif name == "s8":
        host = torch.from_numpy(rng.integers(-128, 128, (distinct, 2 * FULL), dtype=np.int8))
    else:
        host = torch.from_numpy(rng.integers(-32768, 32768, (distinct, 2 * FULL), dtype=np.int16))
    return host.cuda().repeat((frames + distinct - 1) // distinct, 1)[:frames].contiguous()


def part1(repeats, launches=5):
    eng = ksa.SpectrumEngine(N, full_size=FULL, non_overlap=Q, window=WIN, xres=512, max_frames=FRAMES,
                             stream=torch.cuda.current_stream().cuda_stream)
    out = torch.empty((FRAMES, N), dtype=torch.float32, device="cuda")
    iq = {name: device_blocks(name, FRAMES) for name, _ in FORMATS}
    for name, code in FORMATS:
        for _ in range(2):
            eng.curscan_dev(iq[name], code, FRAMES, out, out_mode=ksa.OUT_DB)
    torch.cuda.synchronize()
    rate = {name: [] for name, _ in FORMATS}
    for _ in range(repeats):
        for name, code in FORMATS:
            eng.prof_enable(True)
            for _ in range(launches):
                eng.curscan_dev(iq[name], code, FRAMES, out, out_mode=ksa.OUT_DB)
            ms, k = eng.prof_read()
            eng.prof_enable(False)
            rate[name].append(FRAMES * eng.num_windows / (ms / k) / 1e3)
    nwin = eng.num_windows
    eng.close()
    print("# device-resident, fftSize %d, nonOverlap %s, %s, %d blocks of %d samples (%d windows each), dB output, one MI355X," % (N, Q, WIN, FRAMES, FULL, nwin))
    print("# spectrum-stage time (ksa_prof_read, mean of %d launches per run), the four formats alternating %d times" % (launches, repeats))
    print("# %-5s %10s | %9s %9s %9s | %8s %s" % ("fmt", "B/sample", "MFFT/s min", "med", "max", "vs c64", "verdict"))
    med = {k: statistics.median(v) for k, v in rate.items()}
    spread = max(rate["c64"]) - min(rate["c64"])
    for name, _ in FORMATS:
        verdict = "" if name == "c64" else ("ok" if med[name] >= med["c64"] - spread else "SLOWER than c64 - its spread")
        print("  %-5s %10d | %9.2f %9.2f %9.2f | %8.3f %s" % (name, {"c64": 8, "s16": 4}.get(name, 2), min(rate[name]), med[name],
                                                            max(rate[name]), med[name] / med["c64"], verdict))
    print("# c64 spread (max - min) %.2f MFFT/s" % spread)
    sys.stdout.flush()


def part2(repeats):
    cases = (("u8 ", np.uint8, "ksa_frames_u8 (copy in slots)"), ("s8 ", np.int8, "ksa_frames_dev on pinned memory"),
             ("s16", np.int16, "ksa_frames_dev on pinned memory"))
    frames = 2048
    eng = ksa.SpectrumEngine(N, full_size=FULL, non_overlap=Q, window=WIN, xres=512, max_frames=frames)
    bufs = {}
    rng = np.random.default_rng(9)
    for name, dt, _ in cases:
        pb = ksa.PinnedBuffer((frames, 2 * FULL), dt)
        info = np.iinfo(dt)
        pb.array[:64] = rng.integers(info.min, info.max + 1, (64, 2 * FULL), dtype=dt)
        for f in range(64, frames, 64):
            pb.array[f:f + 64] = pb.array[:64]
        bufs[name] = pb
    for name, _, _ in cases:
        eng.frames(bufs[name].array)
    rate = {name: [] for name, _, _ in cases}
    for _ in range(repeats):
        for name, _, _ in cases:
            t0 = time.perf_counter()
            eng.frames(bufs[name].array)          # returns after the engine's stream is synchronised
            rate[name].append(frames * FULL / (time.perf_counter() - t0) / 1e9)
    eng.close()
    print("# host route, fftSize %d, nonOverlap %s, %s, %d blocks of %d samples in page-locked memory per call, wall time of" % (N, Q, WIN, frames, FULL))
    print("# SpectrumEngine.frames (call + synchronise), alternating %d times" % repeats)
    print("# %-4s %-34s | %8s %8s %8s | %s" % ("fmt", "route", "GS/s min", "med", "max", "GB/s over the link (med)"))
    for name, dt, route in cases:
        m = statistics.median(rate[name])
        print("  %-4s %-34s | %8.2f %8.2f %8.2f | %6.2f" % (name, route, min(rate[name]), m, max(rate[name]), m * 2 * np.dtype(dt).itemsize))
    for pb in bufs.values():
        pb.close()


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    part1(reps)
    part2(reps)
