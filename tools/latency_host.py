#!/usr/bin/env python3
"""Host-pointer entry points (the literal drop-in path): frames per second of ksa_frame_c64 / ksa_curscan_c64 /
ksa_frame_u8 including the H2D copy, launches and the synchronise, one block per call; scan passes; the plot hand-off; and
zeroSpan batches from host memory (ksa_frames_c64 / _u8) beside a pinned H2D copy.  `latency_host.py frames`: the batches only
(profiles/host_frames.txt)."""
import importlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ksa_oracle as orc
ksa = importlib.import_module("prgs-sdr-kspecanal_amd")


def _best(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def host_frames():
    """zeroSpan batches from host memory (ksa_frames_c64 / _u8, >= 256 MiB per call) from pageable and page-locked memory, beside
    the per-block loop (ksa_frame_*) and a page-locked H2D copy of the same bytes measured here (the roofline of this leg); then
    the front end on a 1 GiB uint8 capture with frameBatch 1 and 1024."""
    import contextlib, tempfile
    import torch
    kmod = importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")
    for n, q in ((4096, 0.5), (16384, 0.1), (64, 0.1), (65536, 0.25)):
        full = orc.full_size(n, 2.4e6 if n < 65536 else 1e9)
        x1 = orc.synth_iq(full * 4, 5).astype(np.complex64).reshape(4, full)
        for fmt in ("c64", "u8"):
            one = x1 if fmt == "c64" else np.stack([orc.quantize_u8(r * 0.8) for r in x1])
            k = -(-(256 << 20) // one[0].nbytes)
            eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window="hanning", max_frames=k)
            loop = _best(lambda: [eng.frame(one[i % 4]) for i in range(64)], 3) / 64             # per-block loop, pageable
            pageable = np.tile(one, (k // 4 + 1, 1))[:k].copy()
            pinned = ksa.PinnedBuffer(pageable.shape, pageable.dtype)
            pinned.array[...] = pageable
            src = torch.from_numpy(pageable.view(np.uint8).reshape(-1)).pin_memory()
            dst = torch.empty(src.numel(), dtype=torch.uint8, device="cuda")
            h2d = _best(lambda: (dst.copy_(src, non_blocking=True), torch.cuda.synchronize()), 5)
            for label, arr in (("pageable", pageable), ("pinned", pinned.array)):
                dt = _best(lambda: eng.frames(arr), 5)
                print("frames %-3s N=%-6d q=%-4s %-8s %5d x %7d B: %8.1f MS/s %6.2f GB/s over PCIe = %.2f of pinned H2D (%.2f GB/s);"
                      " per-block loop %7.1f MS/s (%.1f us/block) -> x%.1f"
                      % (fmt, n, q, label, k, one[0].nbytes, k * full / dt / 1e6, pageable.nbytes / dt / 1e9, h2d / dt,
                         pageable.nbytes / h2d / 1e9, full / loop / 1e6, loop * 1e6, loop * k / dt))
            pinned.close()
            del src, dst
            eng.close()
    # the front end: a 1 GiB uint8 `file:` capture, plots off
    n = 4096
    full = orc.full_size(n, 2.4e6)
    frames = (1 << 30) // (2 * full)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "capture.bin")
        blk = orc.quantize_u8(orc.synth_iq(full * 16, 6) * 0.7)
        with open(path, "wb") as f:
            f.write(np.zeros(2 * 16 * 1024, np.uint8).tobytes())                                   # the settle read of sdr_setup
            for _ in range(frames // 16):
                f.write(blk.tobytes())
        times = {}
        for batch in (1, 1024):
            argv = ["zeroSpan", "fftSize", str(n), "window", "hanning", "curScanNonOverlap", "0.5", "prgLoopCnt", str(frames),
                    "iqFormat", "u8", "frameBatch", str(batch), "bPltLevels", "false", "bPltHeatMap", "false", "source", "file:" + path]
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(open(os.devnull, "w")):
                d = kmod.main(argv)
            times[batch] = time.perf_counter() - t0
            assert d["fftHMIndex"] == frames % 128
        for batch, dt in times.items():
            print("front end zeroSpan file: 1 GiB uint8, N=%d q=0.5, %d frames, frameBatch %-4d %7.2f s  %8.1f MS/s  %6.2f GB/s"
                  % (n, frames, batch, dt, frames * full / dt / 1e6, (1 << 30) / dt / 1e9))
        print("front end frameBatch 1024 / frameBatch 1: x%.1f" % (times[1] / times[1024]))


if sys.argv[1:] == ["frames"]:
    host_frames()
    sys.exit(0)

for n, q in ((4096, 0.5), (16384, 0.1), (64, 0.1), (65536, 0.25)):
    full = orc.full_size(n, 2.4e6 if n < 65536 else 1e9)
    x = orc.synth_iq(full, 1).astype(np.complex64)
    raw = orc.quantize_u8(x * 0.8)
    eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window="hanning")
    for name, fn, arg in (("frame c64", eng.frame, x), ("frame u8", eng.frame, raw), ("curscan c64", eng.curscan, x)):
        for _ in range(5):
            fn(arg)
        t0 = time.perf_counter(); reps = 200
        for _ in range(reps):
            fn(arg)
        dt = (time.perf_counter() - t0) / reps
        print("N=%-6d q=%-4s %-12s %8.1f us/block  %7.1f MS/s  (%d windows)" % (n, q, name, dt * 1e6, full / dt / 1e6, eng.num_windows))
    eng.close()

# scan passes from host memory (ksa_scan_pass_c64 / _u8): one pass per call, pageable and page-locked capture blocks
for name, n, q, start, end, win in (("fmScan", 16384, 0.1, 88e6, 108e6, "kaiser"), ("quickFullScan", 64, 0.1, 30e6, 1.5e9, "ones")):
    fs = 2.4e6
    end, _ = orc.fixup_scan_range(start, end, fs)
    steps = len(orc.scan_steps(start, end, fs, 0.5))
    total = int((end - start) / fs) * n
    full = orc.full_size(n, fs)
    eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window=win, xres=min(n, 512), max_frames=steps, scan_total_entries=total)
    x = np.tile(orc.synth_iq(full * 4, 2).astype(np.complex64).reshape(4, full), (steps // 4 + 1, 1))[:steps].copy()
    pinned = ksa.PinnedBuffer((steps, full), np.complex64)
    pinned.array[:] = x
    raw = np.stack([orc.quantize_u8(x[s] * 0.8) for s in range(min(steps, 4))])
    raw = np.tile(raw, (steps // 4 + 1, 1))[:steps].copy()
    for label, arg in (("c64 pageable", x), ("c64 pinned", pinned.array), ("u8 pageable", raw)):
        for _ in range(3):
            eng.scan_pass(arg)
        reps = 20
        t0 = time.perf_counter()
        for _ in range(reps):
            eng.scan_pass(arg)
        dt = (time.perf_counter() - t0) / reps
        print("%-13s %-13s %8.1f us/pass  (%d bands of %d samples: %.1f MS/s, %.2f GB/s over PCIe)" %
              (name, label, dt * 1e6, steps, full, steps * full / dt / 1e6, arg.nbytes / dt / 1e9))
    pinned.close()
    eng.close()

# per-frame plot hand-off: the full state + Levels + markers (rounds 1-3) vs ksa_read_view (round 4)
for n, xres in ((4096, 512), (16384, 512), (65536, 512)):
    full = orc.full_size(n, 2.4e6 if n < 65536 else 1e9)
    eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=0.5, window="hanning", xres=xres)
    eng.frame(orc.synth_iq(full, 3).astype(np.complex64))
    def old():
        st = eng.state()
        lv = eng.levels(xres, "AVG")
        idx, lvl = eng.highs(xres, "AVG", "cur", min_sep=0.025 * xres, count=5)
        return sum(st[k].size for k in ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg", "fftHM")) * 4 + lv.size * 4 + 2 * len(idx) * 4
    def new():
        lv, idx, lvl, rows, hm_index = eng.view(xres, "AVG", curve="cur", min_sep=0.025 * xres, count=5, hm_rows=1)
        return (lv.size + rows.size + 2 * len(idx)) * 4
    for name, fn in (("state + levels + highs", old), ("ksa_read_view", new)):
        for _ in range(5):
            nbytes = fn()
        t0 = time.perf_counter(); reps = 200
        for _ in range(reps):
            fn()
        dt = (time.perf_counter() - t0) / reps
        print("hand-off N=%-6d xRes=%d %-24s %8.1f us/frame  %8d bytes over PCIe" % (n, xres, name, dt * 1e6, nbytes))
    eng.close()

host_frames()
