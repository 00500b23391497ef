"""numpy model of the digital down-converter of include/ksa_ddc.h: the oracle of tests/test_ddc_host.py and
tests/test_gpu_ddc.py (the reference has no such stage).  Three models:

- the float64 model of the stream and block forms: integer phase in uint64, np.exp(-2j pi phi), np.convolve;
- an integer model for the exact tests: the mixer at quarter turns by the top two phase bits, samples and taps as int64, one
  division at the end;
- a float32 emulation (sequential sums of fused multiply-adds, forwards or backwards) that the tests use to check their own bounds on the CPU.
"""
import numpy as np

FMT_C64, FMT_U8, FMT_S8, FMT_S16 = 0, 1, 2, 3
TWO64 = 2 ** 64


def unpack(raw, fmt, u8_offset=127.5, u8_scale=127.5):
    """complex128 [n] from the raw samples (complex64 [n], or [2n] I,Q integers), by the exact rule of the header."""
    raw = np.asarray(raw)
    if fmt == FMT_C64:
        return raw.astype(np.complex128).reshape(-1)
    iq = raw.reshape(-1, 2).astype(np.float64)
    if fmt == FMT_U8:
        iq = (iq - u8_offset) / u8_scale
    else:
        iq = iq / (128.0 if fmt == FMT_S8 else 32768.0)
    return iq[:, 0] + 1j * iq[:, 1]


def phases(n, phase_inc, phase0=0):
    """uint64 [n]: phase0 + i * phase_inc in wrapping 64-bit arithmetic."""
    with np.errstate(over="ignore"):
        return np.uint64(phase0 % TWO64) + np.arange(n, dtype=np.uint64) * np.uint64(phase_inc % TWO64)


def piecewise_phases(pieces):
    """uint64 phases of a stream whose tuning changes: pieces = [(n, phase_inc), ...], continuous phase."""
    out, p = [], 0
    for n, inc in pieces:
        out.append(phases(n, inc, p))
        p = (p + n * inc) % TWO64
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint64)


def rotor(phi):
    """complex128 w = (cos 2 pi phi, -sin 2 pi phi) for uint64 phases."""
    return np.exp(-2j * np.pi * (phi.astype(np.float64) / TWO64))


def out_count(n0, n_in, decim):
    """Outputs of a call that brings the stream from n0 to n0 + n_in samples."""
    return -(-(n0 + n_in) // decim) + (-n0 // decim)


def stream(x, taps, decim, phi):
    """complex128: y[m] = sum_k h[k] v[m D - k], v = x * w(phi), v[n < 0] = 0, for every m with m D < len(x)."""
    v = np.asarray(x, dtype=np.complex128) * rotor(phi)
    if not len(v):
        return np.zeros(0, dtype=np.complex128)
    return np.convolve(v, np.asarray(taps, dtype=np.float64))[:len(v):decim]


def blocks(x, taps, decim, phase_inc):
    """complex128 [nblocks][M]: x [nblocks][L]; the phase restarts in every block; out[b][m] = sum_k h[k] v_b[m D + T-1 - k]."""
    x = np.asarray(x, dtype=np.complex128)
    h = np.asarray(taps, dtype=np.float64)
    w = rotor(phases(x.shape[1], phase_inc))
    return np.array([np.convolve(row * w, h)[len(h) - 1:x.shape[1]:decim] for row in x])


def fir_at(v, taps, decim, first, count):
    """complex128 [count]: y[j] = sum_k h[k] v[first + j D - k], v[n < 0] = 0 -- the outputs of np.convolve(v, h) at
    first + j D, gathered one dot product each (what the large shapes can afford)."""
    h = np.asarray(taps, dtype=np.float64)
    pad = np.concatenate([np.zeros(len(h), dtype=np.complex128), np.asarray(v, dtype=np.complex128)])
    at = len(h) + first + decim * np.arange(count)
    out = np.empty(count, dtype=np.complex128)
    step = max(1, (1 << 22) // len(h))
    for lo in range(0, count, step):
        idx = at[lo:lo + step, None] - np.arange(len(h))[None, :]
        out[lo:lo + step] = pad[idx] @ h
    return out


# ------------------------------------------------------------------------------------------ the integer model
def to_int(raw, fmt):
    """(int64 [n][2] of I,Q, scale): the samples as integers over a power of two.  complex64 must hold k / 2^15; uint8 is taken
    with offset 128 and scale 128."""
    raw = np.asarray(raw)
    if fmt == FMT_C64:
        iq = np.stack([raw.real, raw.imag], axis=-1).astype(np.float64).reshape(-1, 2) * 32768.0
        assert np.array_equal(iq, np.round(iq))
        return iq.astype(np.int64), 32768
    iq = raw.reshape(-1, 2).astype(np.int64)
    if fmt == FMT_U8:
        return iq - 128, 128
    return iq, (128 if fmt == FMT_S8 else 32768)


def int_mix(iq, phi):
    """Quarter-turn mixer: the top two bits of the phase pick (1,0), (0,-1), (-1,0), (0,1); every other bit must be zero."""
    assert not np.any(phi & np.uint64(2 ** 62 - 1))
    q = (phi >> np.uint64(62)).astype(np.int64)
    i, r = iq[:, 0], iq[:, 1]
    re = np.choose(q, [i, r, -i, -r])
    im = np.choose(q, [r, -i, -r, i])
    return np.stack([re, im], axis=-1)


def _int_conv(v, h):
    return np.stack([np.convolve(v[:, c], h) for c in (0, 1)], axis=-1)


def int_stream(iq, scale, taps, decim, phi):
    """complex64 of the stream form in exact integer arithmetic; taps int64."""
    v = int_mix(iq, phi)
    y = _int_conv(v, np.asarray(taps, dtype=np.int64))[:len(v):decim]
    return ((y[:, 0] + 1j * y[:, 1]) / scale).astype(np.complex64)


def int_blocks(iq, scale, taps, decim, phase_inc, nblocks, block_len, starts):
    """complex64 [nblocks][M] of the block form; block b is iq[starts[b] : starts[b] + block_len]."""
    h = np.asarray(taps, dtype=np.int64)
    phi = phases(block_len, phase_inc)
    rows = []
    for b in range(nblocks):
        v = int_mix(iq[starts[b]:starts[b] + block_len], phi)
        y = _int_conv(v, h)[len(h) - 1:block_len:decim]
        rows.append(((y[:, 0] + 1j * y[:, 1]) / scale).astype(np.complex64))
    return np.array(rows)


# ------------------------------------------------------------------------------------------ float32 emulation
def _fma(a, b, c):
    """float32 a * b + c with one rounding (the product of two float32 is exact in float64; the second rounding of the sum,
    float64 to float32, moves a result only when it sits within 2^-29 ulp of a tie)."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def f32_mix(x, phi):
    """complex64 v in float32 steps: the top 32 bits of the phase split into the nearest quarter turn and a remainder, the
    remainder's angle, sin and cos in float32, a float32 complex product of one multiply and one fused multiply-add per part,
    the quarter turns as swaps."""
    xr, xi = np.asarray(x.real, dtype=np.float32), np.asarray(x.imag, dtype=np.float32)
    r = ((phi >> np.uint64(32)) + np.uint64(2 ** 29)) % np.uint64(2 ** 32)
    q = (r >> np.uint64(30)).astype(np.int64)
    f = (r & np.uint64(2 ** 30 - 1)).astype(np.int64) - 2 ** 29
    th = (f.astype(np.float32) * np.float32(2 * np.pi * 2.0 ** -32)).astype(np.float32)
    c, s = np.cos(th).astype(np.float32), np.sin(th).astype(np.float32)
    re = _fma(xr, c, (xi * s).astype(np.float32))
    im = _fma(xi, c, -(xr * s).astype(np.float32))
    re, im = np.where(f == 0, xr, re), np.where(f == 0, xi, im)
    return (np.choose(q, [re, im, -re, -im]) + 1j * np.choose(q, [im, -re, -im, re])).astype(np.complex64)


def f32_fir(v, taps, decim, first, count, backwards=False):
    """complex64 [count]: y[j] = sum_k h[k] v[first + j D - k] summed term by term with float32 fused multiply-adds, k ascending (or descending);
    v[n < 0] = 0."""
    h = np.asarray(taps, dtype=np.float32)
    pad = np.concatenate([np.zeros(len(h), dtype=np.complex64), np.asarray(v, dtype=np.complex64)])
    at = len(h) + first + decim * np.arange(count)
    re, im = np.zeros(count, dtype=np.float32), np.zeros(count, dtype=np.float32)
    order = range(len(h) - 1, -1, -1) if backwards else range(len(h))
    for k in order:
        s = pad[at - k]
        re = _fma(h[k], s.real.astype(np.float32), re)
        im = _fma(h[k], s.imag.astype(np.float32), im)
    return (re + 1j * im).astype(np.complex64)


def bound(taps, max_abs_x):
    """The bound of the float tests: (T + 16) 2^-24 sum|h| max|x| -- T 2^-24 is the worst case of a T-term float32 sum in any
    order; the 16 units cover unpack (1), the angle at 2^-25 turn (1.6), sin / cos at a few ulp, the complex product (3) and
    margin."""
    h = np.asarray(taps, dtype=np.float64)
    return (len(h) + 16) * 2.0 ** -24 * np.abs(h).sum() * max_abs_x
