"""numpy model of include/ksa_resamp.h, the oracle of the resampler's tests (the reference has no counterpart).

Definition: zero-stuff x by L, filter by h, keep every M-th value; y[m] = sum_{q<P} h[p + q L] x[n - q] with t = m M,
n = t div L, p = t mod L.  Four forms: the float64 definition (np.convolve on the zero-stuffed input) and its polyphase form; an
exact integer model (int64 sums of small-integer samples times integer numerators of the taps, and the int16 rule in integers);
an evaluator at chosen output indices that forms t in Python ints (far positions); and a float32 emulation of the chain, one
fused multiply-add per tap, q ascending.

Bound of the float test: err(m) <= (P + 2) 2^-24 sum_q |h[p + q L]| |x[n - q]|.  A chain of P fused multiply-adds has the
first-order bound gamma_P sum|h||x| with gamma_P ~ P u, u = 2^-24 (every partial sum is rounded once, the products not at
all); the two further units cover the higher-order terms (P u <= 2^-16) and the conversion of the float64 reference to the
float32 grid in which the result is compared.  It is derived, not measured."""
import numpy as np

TYPE_F32, TYPE_C64 = 0, 1
OUT_SAME, OUT_S16 = 0, 1
U = 2.0 ** -24


def cdiv(a, b):
    return -(-a // b)


def out_count(seen, n, L, M):
    """Outputs of a stream call of n samples after `seen`: ceil((seen + n) L / M) - ceil(seen L / M); Python ints."""
    return cdiv((int(seen) + int(n)) * L, M) - cdiv(int(seen) * L, M)


def block_first(L, M, P):
    return cdiv((P - 1) * L, M)


def block_out_count(block_len, L, M, P):
    return cdiv(int(block_len) * L, M) - block_first(L, M, P)


def definition(x, h, L, M):
    """float64 (or complex128): zero-stuff, np.convolve, keep every M-th; ceil(len(x) L / M) outputs."""
    x = np.asarray(x)
    h = np.asarray(h, dtype=np.float64)
    n = len(x)
    if n == 0:
        return np.zeros(0, dtype=np.result_type(x.dtype, np.float64))
    z = np.zeros(n * L, dtype=np.result_type(x.dtype, np.float64))
    z[::L] = x
    return np.convolve(z, h)[:n * L:M]


def _gather(x, idx):
    """x[idx] with zero where idx < 0."""
    return np.where(idx >= 0, x[np.clip(idx, 0, None)], 0)


def at(x, h, L, M, ms, origin=0, dtype=np.float64):
    """The polyphase form at output indices ms (Python ints or an integer array): x[0] is sample `origin` of the stream,
    samples before it are zero.  t is formed in Python ints, so that m M may leave 64 bits."""
    x = np.asarray(x)
    h = np.asarray(h)
    P = len(h) // L
    ms = [int(m) for m in np.asarray(ms, dtype=object).reshape(-1)]
    n = np.array([(m * M) // L - int(origin) for m in ms], dtype=np.int64)
    p = np.array([(m * M) % L for m in ms], dtype=np.int64)
    assert len(ms) == 0 or n.max() < len(x), "an output needs a sample that has not arrived"
    acc = np.zeros(len(ms), dtype=np.result_type(x.dtype, dtype))
    for q in range(P):
        acc = acc + h[p + q * L].astype(dtype) * _gather(x, n - q)
    return acc


def polyphase(x, h, L, M):
    """float64: every output of the stream x, by the polyphase form."""
    return at(np.asarray(x, dtype=np.result_type(np.asarray(x).dtype, np.float64)), np.asarray(h, dtype=np.float64), L, M,
              np.arange(cdiv(len(x) * L, M)))


def blocks(x, h, L, M):
    """float64 [nblocks][J]: the block form on the rows of x."""
    x = np.atleast_2d(x)
    P = len(h) // L
    first, J = block_first(L, M, P), block_out_count(x.shape[1], L, M, P)
    return np.array([at(row.astype(np.result_type(row.dtype, np.float64)), np.asarray(h, dtype=np.float64), L, M,
                        np.arange(first, first + J)) for row in x])


# -- exact: small-integer samples, taps num / den with den a power of two ---------------------------------------------------
def exact_taps(rng, T, kind):
    """(float32 taps, int64 numerators, denominator): small integers ("int") or multiples of 1/8 ("pow2")."""
    num = rng.integers(-8, 9, T).astype(np.int64)
    den = 1 if kind == "int" else 8
    return (num / den).astype(np.float32), num, den


def exact_samples(rng, n, cplx=False):
    """Small integers, exact in float32; complex64 with integer parts when cplx."""
    re = rng.integers(-32, 33, n)
    if not cplx:
        return re.astype(np.float32)
    return (re + 1j * rng.integers(-32, 33, n)).astype(np.complex64)


def _int_parts(x):
    x = np.asarray(x)
    if np.iscomplexobj(x):
        return np.rint(x.real).astype(np.int64), np.rint(x.imag).astype(np.int64)
    return (np.rint(x).astype(np.int64),)


def exact_at(x, num, den, L, M, ms, origin=0, out_fmt=OUT_SAME, pcm_scale=1.0):
    """Bit-exact expected outputs at indices ms for integer-valued x: int64 sums of num[p + q L] x[n - q], then / den
    (float32 or complex64, exact while |sum| < 2^24) or the int16 rule applied in integers (pcm_scale a power of two)."""
    P = len(num) // L
    ms = [int(m) for m in np.asarray(ms, dtype=object).reshape(-1)]
    n = np.array([(m * M) // L - int(origin) for m in ms], dtype=np.int64)
    p = np.array([(m * M) % L for m in ms], dtype=np.int64)
    assert len(ms) == 0 or n.max() < len(x)
    sums = []
    for part in _int_parts(x):
        acc = np.zeros(len(ms), dtype=np.int64)
        for q in range(P):
            acc += num[p + q * L] * _gather(part, n - q)
        assert len(ms) == 0 or np.abs(acc).max() < 2 ** 24
        sums.append(acc)
    if out_fmt == OUT_S16:
        return exact_pcm(sums[0], den, pcm_scale)
    if len(sums) == 2:
        return (sums[0] / den + 1j * (sums[1] / den)).astype(np.complex64)
    return (sums[0] / den).astype(np.float32)


def exact_pcm(num, den, pcm_scale):
    """min(max(rint(num / den * pcm_scale), -32768), 32767) in integers: round half to even."""
    scale = int(round(float(pcm_scale) * 1024))                  # pcm_scale a multiple of 1/1024
    assert scale == float(pcm_scale) * 1024
    a, b = np.asarray(num, dtype=np.int64) * scale, int(den) * 1024
    fl, rem = a // b, a % b
    up = (2 * rem > b) | ((2 * rem == b) & (fl % 2 != 0))
    return np.clip(fl + up, -32768, 32767).astype(np.int16)


def exact_stream(x, num, den, L, M, out_fmt=OUT_SAME, pcm_scale=1.0):
    return exact_at(x, num, den, L, M, np.arange(cdiv(len(x) * L, M)), 0, out_fmt, pcm_scale)


def exact_blocks(x, num, den, L, M, starts, block_len, out_fmt=OUT_SAME, pcm_scale=1.0):
    """The model's own block definition on x[s : s + block_len] for every s in starts."""
    P = len(num) // L
    first, J = block_first(L, M, P), block_out_count(block_len, L, M, P)
    return np.array([exact_at(x[s:s + block_len], num, den, L, M, np.arange(first, first + J), 0, out_fmt, pcm_scale)
                     for s in starts])


def pcm(y, pcm_scale):
    """The int16 rule on float values: rint is half to even, NaN becomes 0."""
    p = np.asarray(y, dtype=np.float32) * np.float32(pcm_scale)
    return np.where(np.isnan(p), 0, np.clip(np.rint(p), -32768, 32767)).astype(np.int16)


# -- float32 emulation and the bound ------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """fmaf on float32 arrays: the float64 product of two float32 is exact, the sum is rounded once to float64 and once more to
    float32; the double rounding differs from fmaf only when the float64 sum lands exactly on a float32 tie."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def f32_at(x, h, L, M, ms, origin=0):
    """The chain as the kernel runs it: acc = 0, then acc = fmaf(h[p + q L], x[n - q], acc) for q = 0 .. P-1; the two parts of
    a complex sample have a chain each."""
    x = np.asarray(x)
    h = np.asarray(h, dtype=np.float32)
    P = len(h) // L
    ms = [int(m) for m in np.asarray(ms, dtype=object).reshape(-1)]
    n = np.array([(m * M) // L - int(origin) for m in ms], dtype=np.int64)
    p = np.array([(m * M) % L for m in ms], dtype=np.int64)
    parts = (x.real.astype(np.float32), x.imag.astype(np.float32)) if np.iscomplexobj(x) else (x.astype(np.float32),)
    res = []
    for part in parts:
        acc = np.zeros(len(ms), dtype=np.float32)
        for q in range(P):
            acc = _fma32(h[p + q * L], _gather(part, n - q).astype(np.float32), acc)
        res.append(acc)
    return (res[0] + 1j * res[1]).astype(np.complex64) if len(res) == 2 else res[0]


def bound_at(x, h, L, M, ms, origin=0):
    """(P + 2) 2^-24 sum_q |h[p + q L]| |x[n - q]| at output indices ms; for complex x, per part (real, imag)."""
    x = np.asarray(x)
    h = np.abs(np.asarray(h, dtype=np.float64))
    P = len(h) // L
    parts = (np.abs(x.real), np.abs(x.imag)) if np.iscomplexobj(x) else (np.abs(x),)
    res = [(P + 2) * U * at(part.astype(np.float64), h, L, M, ms, origin) for part in parts]
    return res if len(res) == 2 else res[0]


def worst_ratio(got, want, x, h, L, M, ms, origin=0):
    """max over outputs (and parts) of |got - want| / bound; outputs whose bound is zero must be exact."""
    b = bound_at(x, h, L, M, ms, origin)
    pairs = [(got.real, want.real, b[0]), (got.imag, want.imag, b[1])] if np.iscomplexobj(got) else [(got, want, b)]
    worst = 0.0
    for g, w, bb in pairs:
        err = np.abs(g.astype(np.float64) - w)
        assert np.all(err[bb == 0] == 0)
        if np.any(bb > 0):
            worst = max(worst, float(np.max(err[bb > 0] / bb[bb > 0])))
    return worst
