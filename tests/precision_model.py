"""The fp32 error yardstick of the spectrum kernels -- TEST INFRASTRUCTURE beside test_precision_host.py and test_gpu_precision.py.

Every accuracy bound of those two files is a margin over what a plain single-precision implementation of the same pipeline
loses on the same input:

    metric(device, reference) <= MARGIN * metric(yardstick, reference)

`reference` is the float64 truth (the oracle's curscan, psd_helper.psd, pfb_helper.spectrum).  `yardstick` is the same pipeline
in fp32 on the CPU: window taps rounded to float32, segment times taps in complex64, torch.fft.fft on complex64, torch.abs, one
float32 scale, the fold in float32, fftshift.  It shares no code with the library: the geometry (window starts, scale) comes
from the oracle and the helper modules, never from an engine object.

Host only: numpy, torch on the CPU, oracle/ksa_oracle.py and the two float64 helper modules.
"""
import numpy as np
import torch

import ksa_oracle as orc
import pfb_helper
import psd_helper

# The one device tolerance.  The kernels and the yardstick differ in radix, pass order and summation order; that moves the
# constant of an fp32 FFT's error by a small factor, not its order.  What the tests are there to catch (an approximate
# intrinsic, a twiddle from a neighbouring row, a lost rounding step, a tap from the wrong quarter) moves it by ten or more.
MARGIN = 4.0
# kernel_info()["path"] -> (margin, the arithmetic step that causes it).  A path is listed only with a named cause and a
# derivation, never above 16; every other path stays at MARGIN.  Empty: no path needs one.
PATH_MARGIN = {}

MODES = ("AVG", "MAX", "MIN", "PSD", "PFB")
IMPULSE = 0.5 - 0.25j
TONE_F, TONE_AMP = 0.1173, 0.9
# An impulse frame is held to a per-bin RELATIVE bound only when its true transform magnitude |Y| (before the scale) is at least
# FP32_SAFE and its scaled, folded result at least FP32_TINY.  fp32 forms |Y|^2: below |Y| = 2^-63 the squares are denormal
# (under 2^-126), and to keep 24 good bits they must stay 2^24 above that, |Y| >= 2^-51; 2^-48 leaves three bits more.  A result
# keeps 24 bits down to 2^-126; 2^-102 leaves 24 more.  Only taps far out on the default kaiser window (beta = 64, 3e-27 at its
# ends) put a frame below either; such a frame must read as small as it is.
FP32_SAFE = 2.0 ** -48
FP32_TINY = 2.0 ** -102
LEVEL = 0.1         # the dB check looks at bins at or above LEVEL * rms of the reference
SHARE = 0.95         # ... and those must be at least this share of all bins


def margin(path):
    return PATH_MARGIN.get(path, (MARGIN, ""))[0]


# ------------------------------------------------------------------------------------------------ inputs
def white(total, seed):
    """complex64[total]: complex Gaussian noise of sigma 0.25 per component and no tone, so every bin is a typical bin."""
    return orc.synth_iq(int(total), seed, tones=(), sigma=0.25).astype(np.complex64)


def impulses(frames, full, positions):
    """complex64[frames][full]: frame f holds the one nonzero sample IMPULSE at positions[f % len(positions)].  Every window
    that holds it has an exactly flat spectrum, so each output bin is one chain of twiddle products."""
    x = np.zeros((int(frames), int(full)), dtype=np.complex64)
    pos = np.asarray(positions, dtype=np.int64)
    x[np.arange(frames), pos[np.arange(frames) % len(pos)]] = IMPULSE
    return x


def tone(total, f=TONE_F):
    """complex64[total]: one complex tone of amplitude 0.9 at f cycles per sample, no noise."""
    return (TONE_AMP * np.exp(2j * np.pi * f * np.arange(int(total), dtype=np.float64))).astype(np.complex64)


# ------------------------------------------------------------------------------------------------ impulse positions
def mr_radices(n):
    """The pass radices of the mixed-radix plan for N = 4 * 2^a * 3^b * 5^c, first pass first: the fives, the threes, a // 2
    fours, a two when a is odd, and a last four."""
    m, cnt = n // 4, {}
    for f in (2, 3, 5):
        cnt[f] = 0
        while m % f == 0:
            m //= f
            cnt[f] += 1
    assert n % 4 == 0 and m == 1, n
    return [5] * cnt[5] + [3] * cnt[3] + [4] * (cnt[2] // 2) + [2] * (cnt[2] % 2) + [4]


def digit_radices(n):
    """The digits an input index of an N-point transform is split into, least significant first: base 16 for a power of two
    (the last digit takes what is left), the plan's pass radices otherwise."""
    if n & (n - 1):
        return mr_radices(n)
    r, m = [], n
    while m > 1:
        r.append(min(16, m))
        m //= r[-1]
    return r


def digits(p, radices):
    out = []
    for r in radices:
        out.append(p % r)
        p //= r
    return out


def impulse_positions(n, seed=0):
    """Positions within one window (the caller adds the window's start).  N <= 16384: d * (product of the earlier radices) for every digit and every nonzero
    value d of it, then 1, N - 1 and four seeded random ones.  Above: eight seeded positions whose every digit is nonzero, then
    1 and N - 1."""
    rng = np.random.default_rng(9000 + n + seed)
    radices = digit_radices(n)
    pos = []
    if n <= 16384:
        weight = 1
        for r in radices:
            pos += [d * weight for d in range(1, r)]
            weight *= r
        pos += [1, n - 1] + [int(v) for v in rng.integers(0, n, 4)]
    else:
        for _ in range(8):
            p, weight = 0, 1
            for r in radices:
                p += int(rng.integers(1, r)) * weight
                weight *= r
            pos.append(p)
        pos += [1, n - 1]
    assert all(0 <= p < n for p in pos)
    return pos


# ------------------------------------------------------------------------------------------------ geometry, from the oracle side
def geometry(mode, n, full, q, win):
    """(window starts, float64 scale) of one block of `full` samples; PFB: one start per tap segment."""
    w = np.asarray(win, dtype=np.float64)
    if mode == "PSD":
        starts = psd_helper.geometry(full, n, q)[2]
        return starts, psd_helper.scale(w, len(starts))
    if mode == "PFB":
        return np.arange(len(w) // n, dtype=np.int64) * n, pfb_helper.scale(w)
    return orc.window_starts(full, n, q), orc.win_adj(w) * 2 / n


def reference(x, n, win, mode="AVG", q=None):
    """float64[n]: the truth for one block `x` (complex; PFB: the P * n samples of one frame)."""
    x = np.asarray(x).astype(np.complex128)
    if mode == "PSD":
        return psd_helper.psd(x, n, q, win)
    if mode == "PFB":
        return pfb_helper.spectrum(x, n, win)
    return orc.curscan(x, n, q, np.asarray(win, dtype=np.float64), mode)


def yardstick(x, n, win, mode="AVG", q=None):
    """float32[n]: the same block through the fp32 model."""
    x32 = torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(np.complex64)))
    w32 = torch.from_numpy(np.asarray(win, dtype=np.float64).astype(np.float32))
    starts, scale = geometry(mode, n, len(x32), q, win)
    s32 = np.float32(scale)
    if mode == "PFB":
        y = torch.zeros(n, dtype=torch.complex64)
        for k, s in enumerate(starts):
            y = y + x32[s:s + n] * w32[k * n:(k + 1) * n]
        mag = torch.abs(torch.fft.fft(y)).numpy()
        assert mag.dtype == np.float32
        return np.fft.fftshift(mag * s32)
    segs = torch.stack([x32[s:s + n] for s in starts]) * w32
    y = torch.fft.fft(segs)
    assert y.dtype == torch.complex64
    if mode == "PSD":
        re, im = y.real.numpy(), y.imag.numpy()
        acc = np.zeros(n, dtype=np.float32)
        for k in range(len(starts)):
            acc = acc + (re[k] * re[k] + im[k] * im[k])
        out = acc * s32
    else:
        mag = torch.abs(y).numpy() * s32
        out = mag[0].copy()
        for k in range(1, len(starts)):
            if mode == "AVG":
                out = (out + mag[k]) / np.float32(2)
            elif mode == "MAX":
                out = np.maximum(out, mag[k])
            elif mode == "MIN":
                out = np.minimum(out, mag[k])
            else:
                raise ValueError(mode)
    assert out.dtype == np.float32
    return np.fft.fftshift(out)


def to_db(lin, gain):
    """The engine's formula at the precision of its argument: 10 * log10(x) - gain."""
    lin = np.asarray(lin)
    with np.errstate(divide="ignore", invalid="ignore"):
        if lin.dtype == np.float32:
            return np.float32(10) * np.log10(lin) - np.float32(gain)
        return 10 * np.log10(lin) - gain


# ------------------------------------------------------------------------------------------------ metrics
def _d(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.all(np.isfinite(got)), "shape or non-finite value"
    return got - want, want


def rms_err(got, want):
    d, want = _d(got, want)
    return float(np.linalg.norm(d) / np.linalg.norm(want))


def max_err(got, want):
    d, want = _d(got, want)
    return float(np.max(np.abs(d)) / np.sqrt(np.mean(want * want)))


def floor_err(got, want):
    d, want = _d(got, want)
    return float(np.max(np.abs(d)) / np.max(want))


def bin_err(got, want):
    """max |got / want - 1| over the bins; a bin whose truth is exactly zero (a tap that is exactly zero) must read zero."""
    d, want = _d(got, want)
    zero = want == 0
    assert np.all(np.asarray(got)[zero] == 0), "nonzero value where the truth is exactly zero"
    if zero.all():
        return 0.0
    return float(np.max(np.abs(d[~zero] / want[~zero])))


def impulse_err(got, want, scale):
    """(max |got / want - 1| over all bins of the frames that fp32 can hold to a relative bound, how many frames those are).
    got, want: [frames][n], every row of `want` flat.  The other frames (see FP32_SAFE) must read as small as they are."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.all(np.isfinite(got)) and np.all(got >= 0)
    level = np.max(want, axis=1)
    safe = (level >= FP32_SAFE * scale) & (level >= FP32_TINY)
    assert np.all(got[~safe] <= 2 * max(FP32_SAFE * scale, FP32_TINY)), "a frame below fp32's range does not read as small"
    if not safe.any():
        return 0.0, 0
    return float(np.max(np.abs(got[safe] / want[safe] - 1))), int(np.sum(safe))


def far_bins(want, n):
    """Mask of the bins more than 64 bins (N / 8 below N = 1024) away from the strongest bin of `want`, cyclically."""
    guard = 64 if n >= 1024 else n // 8
    k = np.arange(n)
    dist = np.abs(k - int(np.argmax(want)))
    return np.minimum(dist, n - dist) > guard


def spur(got, want, n):
    """Strongest bin of `got` away from the peak, relative to the true peak: the spur-free range as a ratio."""
    return float(np.max(np.asarray(got, dtype=np.float64)[far_bins(want, n)]) / np.max(want))


def typical_bins(want):
    """Mask of the bins at or above LEVEL * rms of the reference."""
    want = np.asarray(want, dtype=np.float64)
    return want >= LEVEL * np.sqrt(np.mean(want * want))


def db_err(got_db, want_db, mask):
    d = np.abs(np.asarray(got_db, dtype=np.float64)[mask] - np.asarray(want_db, dtype=np.float64)[mask])
    return float(np.max(d))


def within(device, model, path=None):
    """The rule.  Returns (ok, ratio)."""
    ratio = device / model if model > 0 else (0.0 if device == 0 else float("inf"))
    return ratio <= margin(path), ratio
