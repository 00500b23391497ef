#!/usr/bin/env python3
"""Mask check pass at the headline shape: mask_sweep.py [repeats] > profiles/mask_sweep.txt

ksm_check_rows_dev on 65 536 rows of 4096 bins (config 2's per-step cur_db, 1 GiB), on the dB rows the engine itself produces
from bench.py's synthetic source (256 distinct blocks, tiled as bench.py tiles them), with (a) a line nothing crosses (the
rows' own maximum + 10 dB), (b) the same line and 1 % of the rows crossing it at one bin, (c) a line every row crosses at
every bin, the worst case.  Beside them, from the same run: a device-to-device hipMemcpyAsync of the same 1 GiB (it moves
twice the bytes) and ksd_add_rows_dev (256 levels x 4096 columns) on the same rows, which streams the same bytes.  The per-row
part of the pass (scratch clear, count and scatter kernels) is timed on 65 536 rows of 16 bins, where it is all but alone.
One process, one GPU; after 3 warm-up launches every case is launched `repeats` times between two HIP events on the object's
stream and the median (min .. max) is reported.  The acceptance line: (a) takes no longer than the density pass + 10 %."""
import importlib
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
WARMUP = 3


def engine_rows():
    """float32 [ROWS][N] on the device: the engine's cur_db for bench.py's config-2 blocks."""
    host = orc.synth_iq(FULL * DISTINCT, 20201226 + 2).astype(np.complex64)
    iq = torch.view_as_real(torch.from_numpy(host)).reshape(DISTINCT, FULL, 2).cuda()
    eng = ksa.SpectrumEngine(N, full_size=FULL, non_overlap=0.5, window="hanning", max_frames=DISTINCT)
    db = torch.empty((DISTINCT, N), dtype=torch.float32, device="cuda")
    eng.frames_dev(iq, ksa.FMT_C64, DISTINCT, cur_db=db)
    eng.synchronize()
    eng.close()
    return db.repeat(ROWS // DISTINCT, 1).contiguous(), db.cpu().numpy()


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
    rows, distinct = engine_rows()
    quiet_line = ksa.learn_mask(distinct, 10.0)
    bursts = rows.clone()
    bursts[::100, 1234] = float(quiet_line[1234]) + 50.0         # 1 % of the rows, one bin each, 50 dB over the line
    torch.cuda.synchronize()
    launches = repeats + WARMUP
    print("# mask check pass: ksm_check_rows_dev on %d rows x %d bins (%.2f GiB), one MI355X," % (ROWS, N, ROWS * N * 4 / 2 ** 30))
    print("# median (min .. max) of %d launches between HIP events on the object's stream, after %d warm-up launches." % (repeats, WARMUP))
    dst = torch.empty_like(rows)
    with torch.cuda.stream(stream):
        copy = timed(stream, lambda: dst.copy_(rows, non_blocking=True), repeats)
    del dst
    print("# yardstick 1: device-to-device copy of the same rows (twice the bytes): %.3f ms (%.3f .. %.3f) = %.0f GB/s read + written" % (
        copy + (2 * ROWS * N * 4 / copy[0] / 1e6,)))
    dens = ksa.SpectrumDensity(N, N, 256, -140.0, 0.0, stream=stream.cuda_stream)
    dt = timed(stream, lambda: dens.add_rows_dev(rows, ROWS), repeats)
    assert dens.read()[1] == ROWS * launches
    dens.close()
    print("# yardstick 2: ksd_add_rows_dev (256 levels x %d columns) on the same rows: %.3f ms (%.3f .. %.3f) = %.0f GB/s read" % (
        (N,) + dt + (ROWS * N * 4 / dt[0] / 1e6,)))
    print("# %-26s | %8s %8s %8s | %8s %8s %9s | %10s | %s" % ("case", "ms med", "ms min", "ms max", "GB/s", "x copy", "x density", "events", "kernel_info"))
    med = {}
    for name, data, upper, events in (("a quiet", rows, quiet_line, 0),
                                      ("b 1 % of the rows cross", bursts, quiet_line, len(range(0, ROWS, 100))),
                                      ("c every bin of every row", rows, np.full(N, -1000.0, dtype=np.float32), ROWS)):
        mask = ksa.SpectrumMask(N, upper, stream=stream.cuda_stream)
        t = timed(stream, lambda: mask.check_rows_dev(data, ROWS), repeats)
        hits, seen = mask.hits()
        total = mask.events()[1]
        assert seen == ROWS * launches and total == events * launches, (name, seen, total)
        assert int(hits.sum()) == {0: 0, ROWS: ROWS * N * launches}.get(events, events * launches), name
        med[name] = t[0]
        print("  %-26s | %8.3f %8.3f %8.3f | %8.0f %8.2f %9.2f | %10d | %s" % (
            name, t[0], t[1], t[2], ROWS * N * 4 / t[0] / 1e6, t[0] / copy[0], t[0] / dt[0], events, mask.kernel_info()))
        sys.stdout.flush()
        mask.close()
    narrow = torch.full((ROWS, 16), -90.0, dtype=torch.float32, device="cuda")
    mask = ksa.SpectrumMask(16, np.full(16, -50.0, dtype=np.float32), stream=stream.cuda_stream)
    per_row = timed(stream, lambda: mask.check_rows_dev(narrow, ROWS), repeats)
    assert mask.events()[1] == 0
    mask.close()
    print("# per-row part (scratch clear + count + scatter, timed on %d rows x 16 bins): %.3f ms (%.3f .. %.3f) = %.1f %% of (a)" % (
        (ROWS,) + per_row + (100 * per_row[0] / med["a quiet"],)))
    ok = med["a quiet"] <= 1.10 * dt[0]
    print("# acceptance: (a) %.3f ms %s density pass %.3f ms + 10 %% = %.3f ms: %s" % (
        med["a quiet"], "<=" if ok else ">", dt[0], 1.10 * dt[0], "met" if ok else "MISSED"))


if __name__ == "__main__":
    main()
