#!/usr/bin/env python3
"""CFAR detection pass at the headline shape: detect_sweep.py [repeats] > profiles/detect_sweep.txt

kse_detect_rows_dev on 65 536 rows of 4096 bins (config 2's per-step cur_db, 1 GiB), on the dB rows the engine itself produces
from bench.py's synthetic source (256 distinct blocks, tiled as bench.py tiles them), with train 32, guard 2, 10 dB, CA and
(a) the rows with their tones clipped 5 dB above the row's median, so that nothing is detected, (b) 1 % of the rows holding one
emission, (c) eight emissions in every row, (d) every other bin of every row hot: nbins / 2 emissions per row, a worst case
that is recorded only.  Beside them, from the same run: a device-to-device hipMemcpyAsync of the same 1 GiB (it moves twice
the bytes), ksm_check_rows_dev on the same rows with a line nothing crosses, and the engine's own config-2 frames_dev step that
wrote the rows (65 536 frames of 32 768 samples, 16 GiB of IQ in HBM, cur_db written).  One process, one GPU; after
3 warm-up launches every case is launched `repeats` times between two HIP events on the object's stream and the median
(min .. max) is reported.  The condition for per-frame use: (a), (b) and (c) each take no longer than the engine step."""
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
TRAIN, GUARD, THRESHOLD = 32, 2, 10.0
WARMUP = 3


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
    host = orc.synth_iq(FULL * DISTINCT, 20201226 + 2).astype(np.complex64)
    tile = torch.view_as_real(torch.from_numpy(host)).reshape(DISTINCT, FULL, 2).cuda()
    iq = tile.repeat(ROWS // DISTINCT, 1, 1).contiguous()
    del tile
    eng = ksa.SpectrumEngine(N, full_size=FULL, non_overlap=0.5, window="hanning", max_frames=ROWS, stream=stream.cuda_stream)
    db = torch.empty((ROWS, N), dtype=torch.float32, device="cuda")
    step = timed(stream, lambda: eng.frames_dev(iq, ksa.FMT_C64, ROWS, cur_db=db), repeats)
    eng.synchronize()
    eng.close()
    del iq
    # (a): the engine's rows with their tones clipped 5 dB above each row's median, so that nothing is 10 dB above its floor
    quiet = torch.minimum(db, db.median(dim=1, keepdim=True).values + 5.0).contiguous()
    del db
    probe = ksa.SignalDetector(N, TRAIN, GUARD, THRESHOLD)
    probe.detect_rows_dev(quiet, ROWS)
    assert probe.emissions()[1] == 0, "the quiet rows must be quiet"
    probe.close()
    distinct = quiet[:DISTINCT].cpu().numpy()
    level = float(np.median(distinct))
    one = quiet.clone()
    one[::100, 1234:1237] = level + 40.0                       # 1 % of the rows, one emission of three bins
    eight = quiet.clone()
    for k in range(8):
        eight[:, 300 + 450 * k:303 + 450 * k] = level + 40.0   # eight emissions of three bins in every row
    comb = quiet.clone()
    comb[:, ::2] = level + 40.0                                # every other bin
    torch.cuda.synchronize()
    print("# CFAR detection pass: kse_detect_rows_dev on %d rows x %d bins (%.2f GiB), train %d, guard %d, %.0f dB, CA, one MI355X," % (
        ROWS, N, ROWS * N * 4 / 2 ** 30, TRAIN, GUARD, THRESHOLD))
    print("# median (min .. max) of %d launches between HIP events on the object's stream, after %d warm-up launches." % (repeats, WARMUP))
    dst = torch.empty_like(quiet)
    with torch.cuda.stream(stream):
        copy = timed(stream, lambda: dst.copy_(quiet, non_blocking=True), repeats)
    del dst
    print("# yardstick 1: device-to-device copy of the same rows (twice the bytes): %.3f ms (%.3f .. %.3f) = %.0f GB/s read + written" % (
        copy + (2 * ROWS * N * 4 / copy[0] / 1e6,)))
    mask = ksa.SpectrumMask(N, ksa.learn_mask(distinct, 10.0), stream=stream.cuda_stream)
    mt = timed(stream, lambda: mask.check_rows_dev(quiet, ROWS), repeats)
    assert mask.events()[1] == 0
    mask.close()
    print("# yardstick 2: ksm_check_rows_dev on the same rows, a line nothing crosses: %.3f ms (%.3f .. %.3f) = %.0f GB/s read" % (
        mt + (ROWS * N * 4 / mt[0] / 1e6,)))
    print("# yardstick 3: the engine's config-2 frames_dev step that wrote these rows (%d frames of %d samples, cur_db): %.3f ms (%.3f .. %.3f)" % (
        (ROWS, FULL) + step))
    print("# %-30s | %9s %9s %9s | %7s %8s %8s %8s | %10s | %s" % (
        "case", "ms med", "ms min", "ms max", "GB/s", "x copy", "x mask", "of step", "emissions", "kernel_info"))
    med = {}
    for name, data, per_launch in (("a quiet", quiet, 0), ("b 1 % of the rows, one each", one, len(range(0, ROWS, 100))),
                                   ("c eight in every row", eight, 8 * ROWS), ("d every other bin", comb, ROWS * N // 2)):
        det = ksa.SignalDetector(N, TRAIN, GUARD, THRESHOLD, capacity=4096, stream=stream.cuda_stream)
        t = timed(stream, lambda: det.detect_rows_dev(data, ROWS), 3 if name.startswith("d") else repeats)
        n = (3 if name.startswith("d") else repeats) + WARMUP
        hits, seen = det.hits()
        total = det.emissions()[1]
        assert seen == ROWS * n and total == per_launch * n, (name, seen, total, per_launch * n)
        med[name] = t[0]
        print("  %-30s | %9.3f %9.3f %9.3f | %7.0f %8.2f %8.2f %8.2f | %10d | %s" % (
            name, t[0], t[1], t[2], ROWS * N * 4 / t[0] / 1e6, t[0] / copy[0], t[0] / mt[0], t[0] / step[0], per_launch,
            det.kernel_info()))
        sys.stdout.flush()
        det.close()
    worst = max(med[k] for k in med if not k.startswith("d"))
    ok = worst <= step[0]
    print("# per-frame use: the slowest of (a), (b), (c) %.3f ms %s engine step %.3f ms: %s" % (
        worst, "<=" if ok else ">", step[0], "met" if ok else "MISSED"))


if __name__ == "__main__":
    main()
