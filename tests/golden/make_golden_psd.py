#!/usr/bin/env python3
"""Generate tests/golden/psd_*.npz (the Welch PSD fold, curScanCumuMode psd) by EXECUTING THE REFERENCE with bUsePSD true.

Run only where the reference exists (never on the GPU box, never from tests):

    python tests/golden/make_golden_psd.py

The reference is driven as make_golden.py / make_golden_mr.py drive it (run_reference's seams, ReplaySdr, replay_stream),
under ONE shim: its bUsePSD branch hands matplotlib a float `noverlap` (K:375, K:381), which matplotlib >= 3.8 refuses, so
matplotlib.pyplot.psd is wrapped and `noverlap` is int()-ed before the real routine runs -- the truncation the front end
uses.  Everything else (segmenting, window, scaling, mean, the dB stage, Max / Min / Avg, the waterfall, the scan stitch) is
the reference's own code.  Inputs are orc.synth_iq(full, seed): the fixtures keep the seed and a checksum, not the samples.
Only data is written.
"""
import contextlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from make_golden import orc, run_reference, save, sha, ReplaySdr, SEED0  # noqa: E402
from make_golden_mr import replay_stream  # noqa: E402

import matplotlib.pyplot as plt  # noqa: E402  (after make_golden selected the Agg backend)

WINDOWS = {"ones": np.ones, "hanning": np.hanning, "hamming": np.hamming, "kaiser": lambda n: np.kaiser(n, 64)}


@contextlib.contextmanager
def int_noverlap():
    real = plt.psd

    def psd(x, *a, **kw):
        if "noverlap" in kw:
            kw["noverlap"] = int(kw["noverlap"])
        return real(x, *a, **kw)
    plt.psd = psd
    try:
        yield
    finally:
        plt.psd = real


def ref_psd(ns, block, fft_size, non_overlap, window):
    """The reference's own sdr_curscan on one captured block, bUsePSD true."""
    ReplaySdr.stream = replay_stream([block])
    ReplaySdr.pos = 0
    d = {"fullSize": len(block), "fftSize": fft_size, "curScanNonOverlap": non_overlap, "curScanCumuMode": "AVG",
         "theWin": WINDOWS[window](fft_size), "bUsePSD": True, "sdr": ReplaySdr()}
    with int_noverlap():
        out = ns["sdr_curscan"](d)
    plt.close("all")
    return np.array(out, dtype=np.float64)


def run_main(argv, stream, spy_heatmap=False):
    """One run of the reference's main program with bUsePSD true; returns (gD, array last handed to the heat map or None)."""
    captured = {}
    import matplotlib.image as mimage
    orig_set_data = mimage.AxesImage.set_data

    def spy(self, A):
        captured["hm"] = np.array(A, copy=True)
        return orig_set_data(self, A)
    if spy_heatmap:
        mimage.AxesImage.set_data = spy
    try:
        mod = types.ModuleType("rtlsdr"); mod.RtlSdr = ReplaySdr; sys.modules["rtlsdr"] = mod
        ReplaySdr.stream = np.ascontiguousarray(stream, dtype=np.complex64); ReplaySdr.pos = 0
        mg.builtins.input = lambda *a, **k: ""
        sys.argv = ["kspecanal.py"] + [str(v) for v in argv] + ["bUsePSD", "true", "bPltLevels", "false", "bPltHeatMap", "true"]
        with contextlib.redirect_stdout(io.StringIO()), int_noverlap():
            ns = mg.runpy.run_path(mg.REF)
    finally:
        mimage.AxesImage.set_data = orig_set_data
    assert ReplaySdr.pos == len(ReplaySdr.stream), (ReplaySdr.pos, len(ReplaySdr.stream))
    plt.close("all")
    return ns["gD"], captured.get("hm")


def main():
    ns = run_reference(["zeroSpan", "fftSize", 64, "prgLoopCnt", 1], orc.synth_iq(512, SEED0).astype(np.complex64))

    # ---- sdr_curscan, bUsePSD true: every bin ---------------------------------------------------------------------------
    for n, cases in ((64, (("ones", 0.1), ("kaiser", 1.0))),
                     (512, (("ones", 0.25), ("hanning", 0.25), ("hamming", 0.25), ("kaiser", 0.25), ("hanning", 0.1))),
                     (2400, (("kaiser", 0.1), ("hamming", 0.5))),
                     (4096, (("hanning", 0.5), ("hanning", 0.1), ("ones", 0.25)))):
        full = orc.full_size(n, 2.4e6)
        seed = SEED0 + 900 + n
        x = orc.synth_iq(full, seed).astype(np.complex64)
        out = {"%s_q%s" % (w, str(q).replace(".", "")): ref_psd(ns, x, n, q, w) for w, q in cases}
        save("psd_curscan_n%d" % n, seed=seed, iq_sha256=sha(x), fft_size=n, full=full,
             cases=np.array(["%s %r" % (w, q) for w, q in cases]), **out)
    # ---- one large size (first-stage path): sampled bins -----------------------------------------------------------------
    n, q, window = 32768, 0.5, "hamming"
    full = orc.full_size(n, 2.4e6)
    seed = SEED0 + 900 + n
    x = orc.synth_iq(full, seed).astype(np.complex64)
    y = ref_psd(ns, x, n, q, window)
    idx = np.unique(np.concatenate([np.arange(0, n, n // 256), np.argsort(y)[-32:], np.argsort(y)[:32]]))
    save("psd_curscan_n%d" % n, seed=seed, iq_sha256=sha(x), fft_size=n, full=full, non_overlap=q, window=window,
         idx=idx, psd_at_idx=y[idx], psd_decim=y.reshape(256, -1).sum(axis=1), peak=np.max(y))

    # ---- zeroSpan, bUsePSD true: Fft.* and the waterfall buffer handed to the heat map ----------------------------------
    n, q, frames = 512, 0.5, 6
    full = orc.full_size(n, 2.4e6)
    seed = SEED0 + 1000
    x = orc.synth_iq(full * frames, seed).astype(np.complex64)
    g, hm = run_main(["zeroSpan", "fftSize", n, "window", "hanning", "curScanNonOverlap", q, "prgLoopCnt", frames,
                      "xRes", 128], x, spy_heatmap=True)
    assert g["bUsePSD"] is True and hm is not None
    save("psd_zerospan_n512", seed=seed, iq_sha256=sha(x), fft_size=n, non_overlap=q, window="hanning", frames=frames,
         full=g["fullSize"], gain=g["gain"], xres=g["xRes"], hm=hm.astype(np.float64),
         cur=g["Fft.Cur"], max=g["Fft.Max"], min=g["Fft.Min"], avg=g["Fft.Avg"])

    # ---- a scan of three bands, bUsePSD true, the reference's default curScanNonOverlap 0.1 -----------------------------
    n, passes, fs = 512, 2, 2.4e6
    full = orc.full_size(n, fs)
    b2, _ = orc.fixup_scan_range(100e6, 107.2e6, fs)
    steps = len(orc.scan_steps(100e6, b2, fs, 0.5))
    seed = SEED0 + 1100
    x = orc.synth_iq(full * steps * passes, seed).astype(np.complex64)
    g, _ = run_main(["scan", "startFreq", 100e6, "endFreq", 107.2e6, "fftSize", n, "window", "kaiser", "prgLoopCnt", passes], x)
    assert g["bUsePSD"] is True
    save("psd_scan_3band_n512", seed=seed, iq_sha256=sha(x), fft_size=n, passes=passes, steps=steps, full=g["fullSize"],
         start_freq=g["startFreq"], end_freq=g["endFreq"], sampling_rate=g["samplingRate"], gain=g["gain"],
         min_amp=g["minAmp4Clip"], xres=g["xRes"], window=g["window"], non_overlap=g["curScanNonOverlap"],
         scan_non_overlap=g["scanRangeNonOverlap"], base_is_raw=g["bScanRangeBaseDataIsRaw"],
         cur=g["Fft.Cur"], max=g["Fft.Max"], min=g["Fft.Min"], avg=g["Fft.Avg"], hm=g["fftHM"], hm_index=g["fftHMIndex"])


if __name__ == "__main__":
    main()
