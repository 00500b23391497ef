"""Float64 model of the polyphase filter bank front end (KSA_CUMU_PFB, pfb_taps) -- TEST INFRASTRUCTURE beside the PFB tests.

The two formulas of include/ksa.h, written out with numpy only:
    y[n]     = sum over k < P, in the order k = 0, 1, ..., of x[starts[k] + n] * taps[k*N + n]
    out[bin] = mag_scale * |FFT_N(y)[bin]|       (fftshifted)
The reference has no counterpart; with P = 1 the model IS the oracle's curscan at fullSize = fftSize (test_pfb_host.py).  Its
results feed the oracle's unchanged ZeroSpanState.push / ScanState.run_pass, which take linear spectra.
"""
import numpy as np

import ksa_oracle as orc


def prototype(n, taps, window="hamming"):
    """The default prototype filter, restated: a sinc one bin wide, tapered by the oracle's window table over taps*n points."""
    length = int(n) * int(taps)
    return np.sinc((np.arange(length, dtype=np.float64) - (length - 1) / 2.0) / n) * orc.window_table(window, length)


def scale(taps_table):
    return 2.0 / float(np.sum(np.asarray(taps_table, dtype=np.float64)))


def fold(samples, n, taps_table, starts=None):
    """complex128[n]: the time-domain fold of one block."""
    x = np.asarray(samples, dtype=np.complex128)
    w = np.asarray(taps_table, dtype=np.float64)
    p = len(w) // n
    starts = np.arange(p) * n if starts is None else np.asarray(starts)
    y = np.zeros(n, dtype=np.complex128)
    for k in range(p):
        y = y + x[starts[k]:starts[k] + n] * w[k * n:(k + 1) * n]
    return y


def spectrum(samples, n, taps_table, mag_scale=None, starts=None):
    """float64[n]: the linear, fftshifted PFB spectrum of one block."""
    s = scale(taps_table) if mag_scale is None else mag_scale
    return np.fft.fftshift(np.abs(np.fft.fft(fold(samples, n, taps_table, starts))) * s)


def stream_spectra(stream, n, taps_table, frames, stride=None):
    """float64[frames][n]: frame f is the block of len(taps) samples that starts at f*stride (stride n: the critically sampled
    PFB over one sample stream)."""
    stride = n if stride is None else stride
    full = len(taps_table)
    return np.array([spectrum(stream[f * stride:f * stride + full], n, taps_table) for f in range(frames)])
