#!/usr/bin/env python3
"""Generate tests/golden/mr_*.npz (mixed-radix fftSize: 2^a*3^b*5^c, not a power of two) by EXECUTING THE REFERENCE.

Run only where the reference exists (never on the GPU box, never from tests):

    python tests/golden/make_golden_mr.py

The reference is driven exactly as make_golden.py drives it (run_reference / ref_curscan / save).  One difference: its
sdr_read rounds every read below 2^18 samples up to a power of two and drops the tail (K:343), so the replay stream holds
each capture block padded with zeros to that read size.  Large inputs are not stored: they are orc.synth_iq(full, seed) and
the fixture keeps the seed and a checksum.  Only data is written.
"""
import contextlib
import io
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from make_golden import orc, run_reference, ref_curscan, save, sha, ReplaySdr, SEED0  # noqa: E402

READ_UNIT = 2 ** 18   # gSdrReadUnit


def replay_stream(blocks):
    """The samples the reference's sdr_read consumes for these capture blocks (K:327-347): every tail read below
    READ_UNIT is rounded up to a power of two."""
    out = []
    for b in blocks:
        full = len(b)
        whole, rem = divmod(full, READ_UNIT) if full > READ_UNIT else (0, full)
        out.append(b[:whole * READ_UNIT])
        if rem:
            pad = int(2 ** np.ceil(np.log2(rem)))
            out.append(np.concatenate([b[whole * READ_UNIT:], np.zeros(pad - rem, dtype=np.complex64)]))
    return np.concatenate(out).astype(np.complex64)


def main():
    ns = run_reference(["zeroSpan", "fftSize", 64, "prgLoopCnt", 1], orc.synth_iq(512, SEED0).astype(np.complex64))

    # ---- curscan: four windows x AVG / MAX / MIN / RAW, every bin (small N) or sampled bins (large N) ----------------
    for n, q in ((20, 0.1), (96, 0.25), (240, 0.1), (1000, 0.5), (2400, 0.1)):
        full = orc.full_size(n, 2.4e6)
        x = orc.synth_iq(full, SEED0 + 600 + n).astype(np.complex64)
        out = {}
        for window in ("ones", "hanning", "hamming", "kaiser"):
            for cumu in ("AVG", "MAX", "MIN", "RAW"):
                out["%s_%s" % (window, cumu)] = ref_curscan(ns, replay_stream([x]), n, q, window, cumu, full)
        save("mr_curscan_n%d" % n, iq=x, fft_size=n, non_overlap=q, full=full, **out)
    for n, q, window in ((12000, 0.5, "hanning"), (15360, 0.25, "kaiser")):
        full = orc.full_size(n, 2.4e6)
        seed = SEED0 + 600 + n
        x = orc.synth_iq(full, seed).astype(np.complex64)
        y = ref_curscan(ns, replay_stream([x]), n, q, window, "AVG", full)
        ym = ref_curscan(ns, replay_stream([x]), n, q, window, "MAX", full)
        idx = np.unique(np.concatenate([np.arange(0, n, n // 240), np.argsort(y)[-32:], np.argsort(y)[:32]]))
        save("mr_curscan_n%d" % n, seed=seed, iq_sha256=sha(x), fft_size=n, non_overlap=q, window=window, full=full,
             idx=idx, avg_at_idx=y[idx], max_at_idx=ym[idx], avg_decim=y.reshape(240, -1).sum(axis=1),
             max_decim=ym.reshape(240, -1).max(axis=1), peak=np.max(y))

    # ---- zeroSpan fftSize 2400 (xRes 512 -> 300): Fft.* and the waterfall buffer handed to the heat map -------------
    n, q, frames = 2400, 0.5, 260
    full = orc.full_size(n, 2.4e6)
    seed = SEED0 + 700
    x = orc.synth_iq(full * frames, seed).astype(np.complex64).reshape(frames, full)
    captured = {}
    import matplotlib.image as mimage
    orig_set_data = mimage.AxesImage.set_data

    def spy(self, A):
        captured["hm"] = np.array(A, copy=True)
        return orig_set_data(self, A)
    mimage.AxesImage.set_data = spy
    try:
        mod = types.ModuleType("rtlsdr"); mod.RtlSdr = ReplaySdr; sys.modules["rtlsdr"] = mod
        ReplaySdr.stream = replay_stream(x); ReplaySdr.pos = 0
        mg.builtins.input = lambda *a, **k: ""
        sys.argv = ["kspecanal.py", "zeroSpan", "fftSize", str(n), "window", "hanning", "curScanNonOverlap", str(q),
                    "prgLoopCnt", str(frames), "bPltLevels", "false", "bPltHeatMap", "true"]
        with contextlib.redirect_stdout(io.StringIO()):
            nsh = mg.runpy.run_path(mg.REF)
    finally:
        mimage.AxesImage.set_data = orig_set_data
    assert ReplaySdr.pos == len(ReplaySdr.stream)
    g = nsh["gD"]
    assert g["xRes"] == 300, g["xRes"]
    save("mr_zerospan_n2400", seed=seed, iq_sha256=sha(x), fft_size=n, non_overlap=q, window="hanning", frames=frames,
         full=g["fullSize"], gain=g["gain"], xres=g["xRes"], hm=captured["hm"].astype(np.float32),
         cur=g["Fft.Cur"], max=g["Fft.Max"], min=g["Fft.Min"], avg=g["Fft.Avg"])

    # ---- a narrow scan at fftSize 2400, scanRangeNonOverlap 0.5 (hop 1200), three bands -------------------------------
    argv = ["scan", "startFreq", 100e6, "endFreq", 107.2e6, "fftSize", n, "window", "hanning", "prgLoopCnt", 2,
            "scanRangeNonOverlap", 0.5]
    passes, fs = 2, 2.4e6
    b2, _ = orc.fixup_scan_range(100e6, 107.2e6, fs)
    steps = len(orc.scan_steps(100e6, b2, fs, 0.5))
    seed = SEED0 + 800
    x = orc.synth_iq(full * steps * passes, seed).astype(np.complex64).reshape(steps * passes, full)
    mod = types.ModuleType("rtlsdr"); mod.RtlSdr = ReplaySdr; sys.modules["rtlsdr"] = mod
    ReplaySdr.stream = replay_stream(x); ReplaySdr.pos = 0
    sys.argv = ["kspecanal.py"] + [str(v) for v in argv] + ["bPltLevels", "false", "bPltHeatMap", "true"]
    with contextlib.redirect_stdout(io.StringIO()):
        nss = mg.runpy.run_path(mg.REF)
    g = nss["gD"]
    assert ReplaySdr.pos == len(ReplaySdr.stream)
    save("mr_scan_3band_n2400", seed=seed, iq_sha256=sha(x), fft_size=n, passes=passes, steps=steps, full=g["fullSize"],
         start_freq=g["startFreq"], end_freq=g["endFreq"], sampling_rate=g["samplingRate"], gain=g["gain"],
         min_amp=g["minAmp4Clip"], xres=g["xRes"], window=g["window"], non_overlap=g["curScanNonOverlap"],
         scan_non_overlap=g["scanRangeNonOverlap"], base_is_raw=g["bScanRangeBaseDataIsRaw"],
         cur=g["Fft.Cur"], max=g["Fft.Max"], min=g["Fft.Min"], avg=g["Fft.Avg"], hm=g["fftHM"], hm_index=g["fftHMIndex"])

    # ---- what the reference's handle_args leaves for `zeroSpan fftSize 2400` (K:778-949, xRes fix-up K:941-949) -------
    keys = ["prgMode", "fftSize", "xRes", "fullSize", "curScanNonOverlap", "window", "startFreq", "endFreq"]
    gz = run_reference(["zeroSpan", "fftSize", 2400, "window", "hanning", "prgLoopCnt", 0], np.zeros(1, dtype=np.complex64))["gD"]
    cli = {"zerospan_2400": {"argv": ["zeroSpan", "fftSize", "2400", "window", "hanning"],
                             "d": {k: (float(gz[k]) if isinstance(gz[k], (float, np.floating)) else gz[k]) for k in keys}}}
    with open(os.path.join(HERE, "mr_cli_args.json"), "w") as f:
        json.dump(cli, f, indent=1, sort_keys=True)
    print("wrote mr_cli_args.json")


if __name__ == "__main__":
    main()
