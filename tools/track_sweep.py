#!/usr/bin/env python3
"""Linking pass at the size a full detector buffer has:
track_sweep.py [repeats] [out file, default profiles/track_sweep.txt] [a libksa_track.so built with -DKTR_LINK_GLOBAL_ONLY]

ktr_link_dev on n = 2^20 spans in device memory (32 MiB of records) for three shapes of list: sparse singletons (one span every
other row: no pair is adjacent, every search ends at once), the random mix of the tests (rows x 64 bins occupied with p = 0.18,
row_gap 1, bin_slop 1: singletons beside components of dozens of spans) and one long chain (one span per row, each overlapping
the next: one component of 2^20 spans, the deepest parent chain and every reduction on one root).  The call is the eight
launches of a link, so the figure is what the caller waits for.  One process, one GPU; after 3 warm-up links every case is
linked `repeats` times between two HIP events on the object's stream and the median (min .. max) is reported, beside the time of
a device-to-device copy of the same 32 MiB measured the same way: the yardstick of a pass that is bound by nothing but moving
the list once.  The clock state is noted as rocm-smi reports it, read only.

The A/B of the link kernel: the library unites the edges inside a workgroup's 256 spans in LDS and sends memory only what
leaves the tile ("tile").  With a third argument, a second build of csrc_track/ktr_api.hip with build.py's flags and
-DKTR_LINK_GLOBAL_ONLY, in which every edge is united in memory ("global"), every shape is linked with both and the results
are checked to be the same bytes."""
import importlib
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ksa = importlib.import_module("prgs-sdr-kspecanal_amd")
track = importlib.import_module("prgs-sdr-kspecanal_amd.track")

N = 1 << 20
NBINS = 64
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


def clock_state():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showperflevel"], capture_output=True, text=True, timeout=30)
        lines = [ln.strip() for ln in r.stdout.splitlines() if "GPU[0]" in ln and ("sclk" in ln or "mclk" in ln or "Performance" in ln)]
        return "; ".join(lines) if lines else "not reported by rocm-smi"
    except (OSError, subprocess.SubprocessError) as e:
        return "not read (%s)" % type(e).__name__


def records(row, lo, hi, rng):
    s = np.zeros(len(row), dtype=ksa.SPAN_DTYPE)
    s["row"], s["bin_lo"], s["bin_hi"], s["peak_bin"], s["ndet"] = row, lo, hi, lo, hi - lo + 1
    s["peak_db"] = (np.round(rng.normal(-60, 6, len(s)) * 4) / 4).astype(np.float32)
    s["floor_db"] = s["peak_db"] - np.float32(12.5)
    return s


def singletons(rng):
    lo = rng.integers(0, NBINS - 4, N)
    return records(2 * np.arange(N, dtype=np.int64), lo, lo + rng.integers(0, 4, N), rng), 0, 0


def random_mix(rng):
    rows = int(N / (NBINS * 0.18 * 0.82)) + 2048
    occ = np.zeros((rows, NBINS + 2), dtype=np.int8)
    occ[:, 1:-1] = rng.random((rows, NBINS)) < 0.18
    edge = np.diff(occ, axis=1)                                     # +1 where a run starts, -1 one past its end
    r_lo, c_lo = np.nonzero(edge == 1)
    r_hi, c_hi = np.nonzero(edge == -1)
    assert np.array_equal(r_lo, r_hi) and len(r_lo) >= N
    return records(r_lo[:N].astype(np.int64), c_lo[:N], c_hi[:N] - 1, rng), 1, 1


def chain(rng):
    r = np.arange(N, dtype=np.int64)
    return records(r, 20 + r % 3, 24 + r % 5, rng), 0, 0


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 11
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "track_sweep.txt")
    builds = [("tile", track.lib())] + ([("global", track.load(sys.argv[3]))] if len(sys.argv) > 3 else [])
    assert repeats >= 10, "a median of at least 10 launches"
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(20241020)
    out = []

    def say(line):
        print(line)
        sys.stdout.flush()
        out.append(line)

    say("# linking pass: ktr_link_dev on n = %d spans (%d MiB of records) in device memory, %d bins, capacity 2^20 tracks, no labels out," % (
        N, N * 32 >> 20, NBINS))
    say("# one MI355X, median (min .. max) of %d links between HIP events on the object's stream, after %d warm-up links." % (repeats, WARMUP))
    say("# copy ms = a device-to-device copy of the same %d MiB, measured the same way; x copy = link ms / copy ms." % (N * 32 >> 20))
    say("# clock state: %s" % clock_state())
    say("# link: tile = edges inside a workgroup's 256 spans united in LDS, the rest in memory (the library); global = every edge "
        "united in memory (-DKTR_LINK_GLOBAL_ONLY)")
    say("# %-10s %6s %3s %4s | %8s %8s %8s | %9s | %8s %7s | %8s %10s | %s" % (
        "shape", "link", "gap", "slop", "ms med", "ms min", "ms max", "Mspans/s", "copy ms", "x copy", "tracks", "components", "kernel_info"))
    for name, make in (("singletons", singletons), ("random mix", random_mix), ("chain", chain)):
        spans, gap, slop = make(rng)
        row_end = int(spans["row"][-1]) + 1
        dev = torch.from_numpy(spans.view(np.uint8).copy()).cuda()
        dst = torch.empty_like(dev)
        with torch.cuda.stream(stream):
            c = timed(stream, lambda: dst.copy_(dev), repeats)
        seen = None
        for link, lib in builds:
            track._bind._loaded = lib                                # the object below lives and dies with this build
            trk = ksa.EmissionTracker(NBINS, row_gap=gap, bin_slop=slop, capacity=1 << 20, max_spans=N, stream=stream.cuda_stream)
            torch.cuda.synchronize()
            t = timed(stream, lambda: trk.link_dev(dev, N, None, row_end), repeats)
            rec, total, comps = trk.tracks()
            say("  %-10s %6s %3d %4d | %8.3f %8.3f %8.3f | %9.1f | %8.4f %7.1f | %8d %10d | %s" % (
                name, link, gap, slop, t[0], t[1], t[2], N / t[0] / 1e3, c[0], t[0] / c[0], total, comps, trk.kernel_info()))
            assert (name != "singletons" or total == N) and (name != "chain" or total == 1)
            result = (rec.tobytes(), trk.labels().tobytes())
            assert seen is None or seen == result, "the two builds disagree"
            seen = result
            trk.close()
        track._bind._loaded = builds[0][1]
        del dev, dst
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
