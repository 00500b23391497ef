"""Float64 model of one captured block for ANY caller-chosen geometry -- TEST INFRASTRUCTURE beside the contract tests.

The formulas of include/ksa.h written out with numpy, from the header and not from the geometry generators of engine.py:
`starts` is whatever list the caller hands over (any order, any spacing, duplicates), `taps` whatever table, `mag_scale` whatever
number.  With X_k = FFT_N(x[starts[k] : starts[k] + N] * taps) and m_k = |X_k| (K:391):
    RAW      out = mag_scale * m_last                       the window listed last (K:135-136)
    AVG      a = m_0; a = (a + m_k) / 2 for k = 1, 2, ...   in list order (K:137-139); out = mag_scale * a
    MAX/MIN  out = mag_scale * np.max / np.min over the list (K:140-143)
    PSD      out = mag_scale * sum_k |X_k|^2
    PFB      y[n] = sum_k x[starts[k] + n] * taps[k*N + n] in list order; out = mag_scale * |FFT_N(y)|
    PFB_PSD  K = (full_size - max(starts) - N) // N + 1; y_j as above on x[j*N:]; out = mag_scale * sum_j |FFT_N(y_j)|^2
all fftshifted; then the output mode: LINEAR as is, DB = 10*log10(v) - gain (K:106-112, -inf kept), DB_CLIP = the same behind
clip(v, min_amp) with infinities replaced by 0 (K:640-641).  Sample formats are unpacked on the input side (unpack).
"""
import numpy as np

RAW, AVG, MAX, MIN, PSD, PFB, PFB_PSD = range(7)          # KSA_CUMU_*
LINEAR, DB, DB_CLIP = range(3)                            # KSA_OUT_*
C64, U8, S8, S16 = range(4)                               # KSA_FMT_*


def unpack(raw, fmt, u8_offset=127.5, u8_scale=127.5):
    """The samples a block of format `fmt` holds, complex128: complex64 as is, u8 (b - offset) / scale, s8 b / 128, s16 b / 32768."""
    if fmt == C64:
        return np.asarray(raw).astype(np.complex128)
    v = np.asarray(raw).astype(np.float64)
    if fmt == U8:
        v = (v - u8_offset) / u8_scale
    else:
        v = v / (128.0 if fmt == S8 else 32768.0)
    return v[0::2] + 1j * v[1::2]


def subframes(full_size, n, starts):
    """K of KSA_CUMU_PFB_PSD."""
    return (int(full_size) - int(np.max(starts)) - int(n)) // int(n) + 1


def _fold(x, n, starts, taps):
    y = np.zeros(n, dtype=np.complex128)
    for k, s in enumerate(starts):
        y = y + x[s:s + n] * taps[k * n:(k + 1) * n]
    return y


def power(x, n, starts, taps, mode):
    """The fold before scale and output mode (natural bin order)."""
    x = np.asarray(x, dtype=np.complex128)
    taps = np.asarray(taps, dtype=np.float64)
    starts = [int(s) for s in starts]
    if mode == PFB:
        return np.abs(np.fft.fft(_fold(x, n, starts, taps)))
    if mode == PFB_PSD:
        acc = np.zeros(n)
        for j in range(subframes(len(x), n, starts)):
            acc += np.abs(np.fft.fft(_fold(x[j * n:], n, starts, taps))) ** 2
        return acc
    spectra = [np.fft.fft(x[s:s + n] * taps) for s in starts]
    if mode == PSD:
        acc = np.zeros(n)
        for y in spectra:
            acc += y.real * y.real + y.imag * y.imag
        return acc
    mags = [np.abs(y) for y in spectra]
    if mode == RAW:
        return mags[-1]
    if mode == MAX:
        return np.max(mags, axis=0)
    if mode == MIN:
        return np.min(mags, axis=0)
    if mode == AVG:
        a = mags[0]
        for m in mags[1:]:
            a = (a + m) / 2
        return a
    raise ValueError("unknown cumu_mode %r" % (mode,))


def spectrum(x, n, starts, taps, mag_scale, mode, out_mode=LINEAR, gain=0.0, min_amp=0.0):
    """float64[n]: what the library returns for the block `x` (len(x) = full_size samples, complex)."""
    v = np.fft.fftshift(power(x, n, starts, taps, mode) * float(mag_scale))
    if out_mode == LINEAR:
        return v
    if out_mode == DB_CLIP:
        v = np.clip(v, min_amp, None)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = 10 * np.log10(v) - gain
    if out_mode == DB_CLIP:
        out[np.isinf(out)] = 0
    return out
