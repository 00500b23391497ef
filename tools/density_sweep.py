#!/usr/bin/env python3
"""Density histogram add pass at the headline shape: density_sweep.py [repeats] > profiles/density_sweep.txt

ksd_add_rows_dev on 65 536 rows of 4096 bins (config 2's per-step cur_db, 1 GiB) for (levels, width) = (256, 4096), (256, 512),
(1024, 4096), on (a) the dB rows the engine itself produces from bench.py's synthetic source (256 distinct blocks, tiled as
bench.py tiles them) and (b) constant rows, the worst case for same-address atomics.  Yardsticks: a device-to-device
hipMemcpyAsync of the same 1 GiB timed the same way (it moves twice the bytes), and the config-2 step of the newest
BENCH_*.json.  One process, one GPU; after a warm-up every case is launched `repeats` times between two HIP events on the
object's stream and the median is reported."""
import glob
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
ksa = importlib.import_module("prgs-sdr-kspecanal_amd")
import ksa_oracle as orc  # noqa: E402  (bench.py's synthetic source)

N, FULL, ROWS, DISTINCT = 4096, 32768, 65536, 256
CASES = ((256, 4096), (256, 512), (1024, 4096))
LO, HI = -140.0, 0.0


def engine_rows():
    """float32 [ROWS][N] on the device: the engine's cur_db for bench.py's config-2 blocks."""
    host = orc.synth_iq(FULL * DISTINCT, 20201226 + 2).astype(np.complex64)
    iq = torch.view_as_real(torch.from_numpy(host)).reshape(DISTINCT, FULL, 2).cuda()
    eng = ksa.SpectrumEngine(N, full_size=FULL, non_overlap=0.5, window="hanning", max_frames=DISTINCT)
    db = torch.empty((DISTINCT, N), dtype=torch.float32, device="cuda")
    eng.frames_dev(iq, ksa.FMT_C64, DISTINCT, cur_db=db)
    eng.synchronize()
    eng.close()
    return db.repeat(ROWS // DISTINCT, 1).contiguous()


def timed(stream, fn, repeats, warmup=3):
    for _ in range(warmup):
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


def parent_step_ms():
    files = sorted(glob.glob(os.path.join(ROOT, "BENCH_*.json")))
    if not files:
        return None, None
    rec = json.load(open(files[-1]))
    return rec["parsed"]["ms_per_step"], os.path.basename(files[-1])


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 21
    stream = torch.cuda.Stream()
    data = {"engine": engine_rows(), "constant": torch.full((ROWS, N), -75.0, dtype=torch.float32, device="cuda")}
    torch.cuda.synchronize()
    gib = ROWS * N * 4 / 2 ** 30
    step_ms, step_file = parent_step_ms()
    print("# density add pass: ksd_add_rows_dev on %d rows x %d bins (%.2f GiB), levels over [%g, %g) dB, one MI355X," % (ROWS, N, gib, LO, HI))
    print("# median (min .. max) of %d launches between HIP events on the object's stream, after 3 warm-up launches." % repeats)
    dst = torch.empty_like(data["engine"])
    with torch.cuda.stream(stream):
        copy = timed(stream, lambda: dst.copy_(data["engine"], non_blocking=True), repeats)
    del dst
    print("# yardstick 1: device-to-device copy of the same rows (twice the bytes): %.3f ms (%.3f .. %.3f) = %.0f GB/s read + written" % (
        copy + (2 * ROWS * N * 4 / copy[0] / 1e6,)))
    if step_ms is not None:
        print("# yardstick 2: config-2 step of %s: %.3f ms per %d frames" % (step_file, step_ms, ROWS))
    print("# %-8s %6s %6s | %8s %8s %8s | %8s %9s %8s | %s" % ("rows", "levels", "width", "ms med", "ms min", "ms max", "GB/s", "x copy", "of step", "kernel_info"))
    med = {}
    for levels, width in CASES:
        for name, rows in data.items():
            dens = ksa.SpectrumDensity(N, width, levels, LO, HI, stream=stream.cuda_stream)
            t = timed(stream, lambda: dens.add_rows_dev(rows, ROWS), repeats)
            counts, seen = dens.read()
            assert seen == ROWS * (repeats + 3) and int(counts.sum()) == seen * N
            med[(levels, width, name)] = t[0]
            print("  %-8s %6d %6d | %8.3f %8.3f %8.3f | %8.0f %9.2f %8s | %s" % (
                name, levels, width, t[0], t[1], t[2], ROWS * N * 4 / t[0] / 1e6, t[0] / copy[0],
                "%.1f %%" % (100 * t[0] / step_ms) if step_ms else "-", dens.kernel_info()))
            sys.stdout.flush()
            dens.close()
    for levels, width in CASES:
        print("# constant / engine rows at (%d, %d): %.2f" % (levels, width, med[(levels, width, "constant")] / med[(levels, width, "engine")]))


if __name__ == "__main__":
    main()
