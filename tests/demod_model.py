"""numpy model of the demodulator of include/ksa_demod.h: the oracle of tests/test_demod_host.py and tests/test_gpu_demod.py
(the reference has no such stage).  Three models:

- the float64 model of the stream and block forms: the detector with the axis rule applied explicitly (np.arctan2 alone returns
  -0.5 turn for (-re, -0)), np.convolve;
- an exact model for inputs whose detector values are exact: AM on integer Pythagorean samples, FM and PM on samples A * i^k
  (d in {0, +-0.25, 0.5}); taps that are small integers or powers of two, int64 sums, the int16 rule in integers;
- a float32 emulation (the detector in float32, sequential sums of fused multiply-adds, forwards or backwards) that the tests
  use to check their own bounds on the CPU.
"""
import numpy as np

MODE_AM, MODE_FM, MODE_PM = 0, 1, 2
OUT_F32, OUT_S16 = 0, 1
UNIT = 2.0 ** -24


def lead(mode):
    return 1 if mode == MODE_FM else 0


def out_count(n0, n_in, decim):
    """Outputs of a call that brings the stream from n0 to n0 + n_in samples."""
    return -(-(n0 + n_in) // decim) + (-n0 // decim)


def block_out_count(block_len, ntaps, decim, mode):
    return (block_len - lead(mode) - ntaps) // decim + 1


# ------------------------------------------------------------------------------------------ the float64 model
def turns(re, im):
    """atan2(im, re) / 2 pi in [-0.5, 0.5] with the axes exact; zero means either sign of zero."""
    re, im = np.asarray(re, dtype=np.float64), np.asarray(im, dtype=np.float64)
    t = np.arctan2(im, re) / (2 * np.pi)
    t = np.where(re == 0, np.where(im > 0, 0.25, -0.25), t)
    return np.where(im == 0, np.where(re < 0, 0.5, 0.0), t)


def detect(x, mode):
    """float64 d[n] of the complex samples x; FM takes x[-1] = 0."""
    x = np.asarray(x, dtype=np.complex128).reshape(-1)
    if mode == MODE_AM:
        return np.hypot(x.real, x.imag)
    if mode == MODE_PM:
        return turns(x.real, x.imag)
    p = x * np.conj(np.concatenate([[0], x[:-1]]))
    return turns(p.real, p.imag)


def stream(x, taps, decim, mode):
    """float64: y[m] = sum_k h[k] d[m D - k], d[n < 0] = 0, for every m with m D < len(x)."""
    d = detect(x, mode)
    if not len(d):
        return np.zeros(0)
    return np.convolve(d, np.asarray(taps, dtype=np.float64))[:len(d):decim]


def blocks(x, taps, decim, mode):
    """float64 [nblocks][M]: x [nblocks][L]; out[b][m] = sum_k h[k] d_b[lead + m D + T-1 - k]."""
    x = np.asarray(x, dtype=np.complex128)
    h = np.asarray(taps, dtype=np.float64)
    return np.array([np.convolve(detect(row, mode), h)[lead(mode) + len(h) - 1:x.shape[1]:decim] for row in x])


def fir_at(d, taps, decim, first, count):
    """float64 [count]: y[j] = sum_k h[k] d[first + j D - k], d[n < 0] = 0, one dot product each (what the large shapes can
    afford)."""
    h = np.asarray(taps, dtype=np.float64)
    pad = np.concatenate([np.zeros(len(h)), np.asarray(d, dtype=np.float64)])
    at = len(h) + first + decim * np.arange(count)
    out = np.empty(count)
    step = max(1, (1 << 22) // len(h))
    for lo in range(0, count, step):
        idx = at[lo:lo + step, None] - np.arange(len(h))[None, :]
        out[lo:lo + step] = pad[idx] @ h
    return out


def pcm(y, scale):
    """The int16 rule on float64 values: (int16) min(max(rint(y * scale), -32768), 32767)."""
    return np.clip(np.rint(np.asarray(y, dtype=np.float64) * scale), -32768, 32767).astype(np.int16)


# ------------------------------------------------------------------------------------------ the exact model
PYTHAGOREAN = ((3, 4, 5), (5, 12, 13), (8, 15, 17), (7, 24, 25), (20, 21, 29), (9, 40, 41), (1, 0, 1), (0, 2, 2), (0, 0, 0))


def exact_am_samples(rng, n):
    """(complex64 [n], int64 [n] of |x|): Pythagorean pairs in either order with any signs, times a small integer."""
    t = np.array(PYTHAGOREAN)[rng.integers(0, len(PYTHAGOREAN), n)]
    k = rng.integers(1, 4, n)
    swap = rng.integers(0, 2, n).astype(bool)
    a, b = np.where(swap, t[:, 1], t[:, 0]), np.where(swap, t[:, 0], t[:, 1])
    x = (k * a * rng.choice([-1, 1], n) + 1j * (k * b * rng.choice([-1, 1], n))).astype(np.complex64)
    return x, (k * t[:, 2]).astype(np.int64)


def exact_turn_samples(rng, n):
    """(complex64 [n], int64 [n] of k): samples A * i^k with small integer amplitudes A >= 1, on the axes."""
    k = rng.integers(0, 4, n)
    amp = rng.integers(1, 64, n).astype(np.float64)
    x = (amp * np.array([1, 1j, -1, -1j])[k]).astype(np.complex64)
    return x, k.astype(np.int64)


def exact_detect(mode, mag=None, k=None):
    """(int64 numerators [n], denominator) of the exact detector values: AM |x| over 1; PM and FM quarter turns over 4, with
    2 quarters for half a turn and -1 for three; FM takes x[-1] = 0, which gives 0."""
    if mode == MODE_AM:
        return np.asarray(mag, dtype=np.int64), 1
    k = np.asarray(k, dtype=np.int64)
    q = k % 4
    if mode == MODE_FM:
        q = np.concatenate([[0], (k[1:] - k[:-1]) % 4]) if len(k) else k
    return np.where(q == 3, -1, q).astype(np.int64), 4


def int_taps(taps):
    """(int64 [T], denominator): taps that are integers over a common power of two."""
    t = np.asarray(taps, dtype=np.float64)
    den = 1
    while not np.array_equal(t * den, np.round(t * den)):
        den *= 2
        assert den <= 2 ** 20
    return (t * den).astype(np.int64), den


def _exact_out(num, den, out_fmt, pcm_scale):
    num = np.asarray(num, dtype=np.int64)
    if out_fmt == OUT_F32:
        assert np.all(np.abs(num) < 2 ** 24)                 # the sum is a float32 value
        return (num / den).astype(np.float32)
    scale = int(pcm_scale)
    assert scale == pcm_scale and np.all(np.abs(num) < 2 ** 40) and scale < 2 ** 20
    q, rem = np.divmod(num * scale, den)                     # floor, then half to even
    r = q + (2 * rem > den) + ((2 * rem == den) & (q % 2 == 1))
    return np.clip(r, -32768, 32767).astype(np.int16)


def exact_conv(dn, dden, taps):
    """(int64 numerators of the undecimated filter's outputs over the whole input, denominator): computed once, every stream
    length and every block picks from it -- the filter is causal, so a shorter stream's outputs are a prefix."""
    h, hden = int_taps(taps)
    return np.convolve(np.asarray(dn, dtype=np.int64), h) if len(dn) else np.zeros(0, dtype=np.int64), dden * hden


def exact_stream(dn, dden, taps, decim, out_fmt=OUT_F32, pcm_scale=1.0, conv=None):
    """The stream form in integers: float32 or int16 [ceil(n / D)].  conv: exact_conv of a longer input that starts alike."""
    full, den = exact_conv(dn, dden, taps) if conv is None else conv
    return _exact_out(full[:len(dn):decim], den, out_fmt, pcm_scale)


def exact_blocks(dn, dden, taps, decim, mode, starts, block_len, out_fmt=OUT_F32, pcm_scale=1.0, conv=None):
    """The block form in integers; block b is samples starts[b] .. starts[b] + block_len.  Output m of a block picks the
    undecimated output at start + lead + m D + T-1: its support starts at the block's sample `lead`, where FM's detector value
    is that of the whole input (only a block's first sample, which no output touches, has no predecessor)."""
    full, den = exact_conv(dn, dden, taps) if conv is None else conv
    ntaps = len(np.asarray(taps).reshape(-1))
    return _exact_out(np.array([full[s + lead(mode) + ntaps - 1:s + block_len:decim] for s in starts]), den, out_fmt, pcm_scale)


# ------------------------------------------------------------------------------------------ float32 emulation
def _fma(a, b, c):
    """float32 a * b + c with one rounding (the product of two float32 is exact in float64; the second rounding of the sum,
    float64 to float32, moves a result only when it sits within 2^-29 ulp of a tie)."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def f32_turns(re, im):
    re, im = np.asarray(re, dtype=np.float32), np.asarray(im, dtype=np.float32)
    t = (np.arctan2(im, re).astype(np.float32) * np.float32(1 / (2 * np.pi))).astype(np.float32)
    t = np.clip(t, np.float32(-0.5), np.float32(0.5))
    t = np.where(re == 0, np.where(im > 0, np.float32(0.25), np.float32(-0.25)), t)
    return np.where(im == 0, np.where(re < 0, np.float32(0.5), np.float32(0.0)), t).astype(np.float32)


def f32_detect(x, mode):
    """float32 d[n] in the header's float32 steps."""
    x = np.asarray(x, dtype=np.complex64).reshape(-1)
    xr, xi = x.real.astype(np.float32), x.imag.astype(np.float32)
    if mode == MODE_AM:
        return np.sqrt(_fma(xr, xr, (xi * xi).astype(np.float32))).astype(np.float32)
    if mode == MODE_PM:
        return f32_turns(xr, xi)
    yr, yi = np.concatenate([[np.float32(0)], xr[:-1]]), np.concatenate([[np.float32(0)], xi[:-1]])
    pr = _fma(xr, yr, (xi * yi).astype(np.float32))
    pi = _fma(xi, yr, -(xr * yi).astype(np.float32))
    return f32_turns(pr, pi)


def f32_fir(d, taps, decim, first, count, backwards=False):
    """float32 [count]: y[j] = sum_k h[k] d[first + j D - k] summed term by term with float32 fused multiply-adds, k ascending
    (or descending); d[n < 0] = 0."""
    h = np.asarray(taps, dtype=np.float32)
    pad = np.concatenate([np.zeros(len(h), dtype=np.float32), np.asarray(d, dtype=np.float32)])
    at = len(h) + first + decim * np.arange(count)
    acc = np.zeros(count, dtype=np.float32)
    for k in (range(len(h) - 1, -1, -1) if backwards else range(len(h))):
        acc = _fma(h[k], pad[at - k], acc)
    return acc


def detector_units(mode, max_abs_x):
    """B of the bound: 8 * 2^-24 turn for FM and PM -- the complex product (<= 0.4), a 6-ulp atan2f at pi (3.8), the scale
    (0.5) and margin; 4 * 2^-24 max|x| for AM -- two roundings of the square and one of the root."""
    return 4 * UNIT * max_abs_x if mode == MODE_AM else 8 * UNIT


def bound(taps, mode, max_abs_x):
    """The bound of the float tests: sum|h| ((T + 16) 2^-24 dmax + B), dmax = 0.5 for FM and PM and max|x| for AM; T 2^-24 is
    the worst case of a T-term float32 sum in any order."""
    h = np.asarray(taps, dtype=np.float64)
    dmax = max_abs_x if mode == MODE_AM else 0.5
    return np.abs(h).sum() * ((len(h) + 16) * UNIT * dmax + detector_units(mode, max_abs_x))


def float_input(rng, n, mode):
    """complex64 [n] of the float tests: amplitudes log-uniform in [1e-3, 3e4], phase steps (FM) or phases (PM, AM) within
    +-0.45 turn, so that no wrap can flip a sign under the filter."""
    amp = np.exp(rng.uniform(np.log(1e-3), np.log(3e4), n))
    ang = rng.uniform(-0.45, 0.45, n)
    if mode == MODE_FM:
        ang = np.cumsum(ang)
    return (amp * np.exp(2j * np.pi * ang)).astype(np.complex64)
