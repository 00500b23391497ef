"""Float64 restatement of the Welch PSD fold (curScanCumuMode psd) -- TEST INFRASTRUCTURE beside the PSD tests.

What the reference's `bUsePSD true` branch returns (K:374-384: matplotlib's plt.psd with NFFT = fftSize, the run's window,
noverlap = fftSize*(1 - curScanNonOverlap), Fs = 2 by default; two-sided for complex input, no detrending, scaled as a
density, mean over the segments, fftshifted), written out with numpy only.  `noverlap` is truncated to an int, as the front
end does (matplotlib >= 3.8 refuses the reference's float).  tests/golden/psd_*.npz pin it against runs of the reference
itself (tests/golden/make_golden_psd.py); its results feed the oracle's unchanged ZeroSpanState.push / ScanState.run_pass,
which take linear spectra.
"""
import numpy as np

import ksa_oracle as orc

PSD_FS = 2.0   # plt.psd's default Fs, which K:381 keeps


def geometry(full_size, fft_size, non_overlap):
    """(noverlap, step, segment starts) of mlab.psd for one capture block."""
    noverlap = int(fft_size * (1 - non_overlap))
    step = fft_size - noverlap
    count = (full_size - noverlap) // step
    return noverlap, step, np.arange(count, dtype=np.int64) * step


def scale(win, count, fs=PSD_FS):
    w = np.asarray(win, dtype=np.float64)
    return 1.0 / (fs * np.sum(w * w) * count)


def psd(samples, fft_size, non_overlap, win, fs=PSD_FS):
    """float64[fft_size]: the linear, fftshifted PSD of one capture block."""
    x = np.asarray(samples, dtype=np.complex128)
    w = np.asarray(win, dtype=np.float64)
    _, _, starts = geometry(len(x), fft_size, non_overlap)
    acc = np.zeros(fft_size)
    for s in starts:
        y = np.fft.fft(x[s:s + fft_size] * w)
        acc += y.real * y.real + y.imag * y.imag
    return np.fft.fftshift(acc * scale(w, len(starts), fs))


def fixture_cases(g):
    """(window, nonOverlap, key) of every case a psd_curscan_* fixture holds."""
    for c in g["cases"]:
        w, q = str(c).split()
        yield w, float(q), "%s_q%s" % (w, q.replace(".", ""))


def zerospan_state(g, x=None):
    """ZeroSpanState of the oracle, unchanged, fed with restated PSDs of the zeroSpan fixture's frames."""
    n, q, full, frames = int(g["fft_size"]), float(g["non_overlap"]), int(g["full"]), int(g["frames"])
    if x is None:
        x = orc.synth_iq(full * frames, int(g["seed"])).astype(np.complex64)
    win = orc.window_table(str(g["window"]), n)
    st = orc.ZeroSpanState(n, int(g["xres"]), float(g["gain"]))
    for f in x.reshape(frames, full):
        st.push(psd(f, n, q, win))
    return st, x


def scan_state(g, x=None):
    n, full, passes, steps = int(g["fft_size"]), int(g["full"]), int(g["passes"]), int(g["steps"])
    if x is None:
        x = orc.synth_iq(full * steps * passes, int(g["seed"])).astype(np.complex64)
    win = orc.window_table(str(g["window"]), n)
    st = orc.ScanState(n, float(g["start_freq"]), float(g["end_freq"]), float(g["sampling_rate"]), float(g["gain"]),
                       float(g["min_amp"]), int(g["xres"]), float(g["scan_non_overlap"]))
    for p in x.reshape(passes, steps, full):
        st.run_pass([psd(b, n, float(g["non_overlap"]), win) for b in p])
    return st, x
