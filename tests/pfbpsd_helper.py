"""Float64 model of the integrating polyphase spectrometer (KSA_CUMU_PFB_PSD, pfb_spectra) -- TEST INFRASTRUCTURE beside its tests.

The three formulas of include/ksa.h, written out with numpy on pfb_helper.fold:
    K        = (full_size - max(starts) - N) // N + 1
    y_j[n]   = sum over k < P, in the order k = 0, 1, ..., of x[j*N + starts[k] + n] * taps[k*N + n]        j = 0 .. K-1
    out[bin] = mag_scale * sum over j < K of |FFT_N(y_j)[bin]|^2       (fftshifted)
The reference has no counterpart.  With P = 1 the model IS psd_helper.psd at non-overlap 1.0, with K = 1 it is the square of
pfb_helper.spectrum (test_pfbpsd_host.py).  Its results feed the oracle's unchanged ZeroSpanState.push / ScanState.run_pass,
which take linear spectra.
"""
import numpy as np

import pfb_helper as pfb

PSD_FS = 2.0


def count(full_size, n, taps_table, starts=None):
    """K: the sub-frames a block of full_size samples holds."""
    p = len(taps_table) // n
    last = (p - 1) * n if starts is None else int(np.max(starts))
    return (int(full_size) - last - n) // n + 1


def scale(taps_table, k, fs=PSD_FS):
    """1 / (Fs * sum(taps^2) * K): the density convention of the Welch fold on the long prototype."""
    w = np.asarray(taps_table, dtype=np.float64)
    return 1.0 / (float(fs) * float(np.sum(w * w)) * int(k))


def spectrum(samples, n, taps_table, mag_scale=None, starts=None):
    """float64[n]: the linear, fftshifted integrated power spectrum of one block (its length is full_size)."""
    x = np.asarray(samples, dtype=np.complex128)
    k = count(len(x), n, taps_table, starts)
    s = scale(taps_table, k) if mag_scale is None else mag_scale
    acc = np.zeros(n)
    for j in range(k):
        y = np.fft.fft(pfb.fold(x[j * n:], n, taps_table, starts))
        acc += y.real * y.real + y.imag * y.imag
    return np.fft.fftshift(acc * s)


def stream_spectra(stream, n, taps_table, full_size, blocks, stride):
    """float64[blocks][n]: block b is the full_size samples from b*stride."""
    return np.array([spectrum(stream[b * stride:b * stride + full_size], n, taps_table) for b in range(blocks)])
