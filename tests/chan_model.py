"""numpy model of the polyphase channelizer of include/ksa_chan.h: the oracle of tests/test_chan_host.py and
tests/test_gpu_chan.py (the reference has no such stage).  Four models:

- the definition, written directly in float64: y[c][m] = sum_k h[k] x[m D - k] exp(-2 pi i c (m D - k) / M);
- the polyphase evaluation in float64 (branch sums, an M-point transform, the quarter-turn rotation);
- a float32 emulation of that evaluation: chains of fused multiply-adds (ddc_model._fma), the radix-2 decimation-in-time
  network on bit-reversed input with float32 twiddles and rounded products, rotations by swaps and signs;
- exact integer helpers for channels 0, M/4, M/2 and 3M/4, whose mixer only takes the values 1, -i, -1, i.
"""
import numpy as np

from ddc_model import FMT_C64, FMT_U8, FMT_S8, FMT_S16, _fma, to_int, unpack  # noqa: F401  (re-exported for the tests)


def first_column(M, O, P):
    """ceil((T - 1) / D): the first column whose whole support lies inside a block."""
    D, T = M // O, M * P
    return -(-(T - 1) // D)


def out_count(n0, n_in, D):
    """Columns of a call that brings the stream from n0 to n0 + n_in samples."""
    return -(-(n0 + n_in) // D) + (-n0 // D)


def block_out_count(block_len, M, O, P):
    return (block_len - 1) // (M // O) - first_column(M, O, P) + 1


def block_len_for(F, M, O, P):
    return (M // O) * (first_column(M, O, P) + F - 1) + 1


def _padded(x, T):
    return np.concatenate([np.zeros(T, dtype=np.complex128), np.asarray(x, dtype=np.complex128)])


def definition(x, taps, M, O, cols=None, channels=None):
    """complex128 [len(channels)][len(cols)]: the definition, one mixed dot product per value.  cols default to every m with
    m D < len(x), channels to all M."""
    h = np.asarray(taps, dtype=np.float64)
    T, D = len(h), M // O
    cols = np.arange(-(-len(x) // D)) if cols is None else np.asarray(cols)
    channels = np.arange(M) if channels is None else np.asarray(channels)
    pad = _padded(x, T)
    k = np.arange(T)
    out = np.empty((len(channels), len(cols)), dtype=np.complex128)
    for j, m in enumerate(cols):
        n = m * D - k                                              # sample index of tap k
        seg = pad[T + n] * h
        ph = (np.outer(channels, n) % M) / M                       # exact integer phase, then one division
        out[:, j] = (np.exp(-2j * np.pi * ph) * seg[None, :]).sum(axis=1)
    return out


def branch_sums(x, taps, M, O, cols):
    """complex128 [len(cols)][M]: u_m[p] = sum_q h[p + M q] x[m D - p - M q]."""
    h = np.asarray(taps, dtype=np.float64)
    T, D = len(h), M // O
    pad = _padded(x, T)
    idx = T + np.asarray(cols)[:, None] * D - np.arange(T)[None, :]
    prod = pad[idx] * h[None, :]                                   # [cols][T], k = p + M q
    return prod.reshape(len(cols), T // M, M).sum(axis=1)


def polyphase(x, taps, M, O, cols=None):
    """complex128 [M][len(cols)]: the evaluation of the header in float64."""
    D = M // O
    cols = np.arange(-(-len(x) // D)) if cols is None else np.asarray(cols)
    u = branch_sums(x, taps, M, O, cols)
    z = np.fft.ifft(u, axis=1) * M                                 # sum_p u[p] exp(+2 pi i c p / M)
    c = np.arange(M)
    rot = np.exp(-2j * np.pi * ((np.outer(cols, c) % O) / O))
    return (z * rot).T


# ------------------------------------------------------------------------------------------ float32 emulation
def twiddles(M):
    """complex64 [max(M/2, 1)]: exp(+2 pi i k / M) from float64, rounded once, exact on the axes."""
    k = np.arange(max(M // 2, 1))
    w = np.exp(2j * np.pi * k / M)
    re, im = w.real.astype(np.float32), w.imag.astype(np.float32)
    re[0], im[0] = 1, 0
    if M >= 4:
        re[M // 4], im[M // 4] = 0, 1
    return re, im


def _bitrev(M):
    bits = M.bit_length() - 1
    return np.array([int(format(p, "0%db" % bits)[::-1], 2) for p in range(M)])


def f32_transform(ur, ui, M):
    """float32 re, im [n][M]: z[c] = sum_p u[p] exp(+2 pi i c p / M) by the radix-2 decimation-in-time network; a butterfly is
    a + w b, a - w b with w b = (fma(wr, br, -(wi bi)), fma(wr, bi, wi br))."""
    rev = _bitrev(M)
    re, im = np.empty_like(ur), np.empty_like(ui)
    re[:, rev], im[:, rev] = ur, ui
    wr, wi = twiddles(M)
    hs = 1
    while hs < M:
        i = np.arange(M)
        lo = i[(i & hs) == 0]
        j = lo & (hs - 1)
        tr, ti = wr[j * (M // (2 * hs))], wi[j * (M // (2 * hs))]
        br, bi = re[:, lo + hs], im[:, lo + hs]
        pr = _fma(tr, br, -(ti * bi).astype(np.float32))
        pi = _fma(tr, bi, (ti * br).astype(np.float32))
        ar, ai = re[:, lo].copy(), im[:, lo].copy()
        re[:, lo], im[:, lo] = ar + pr, ai + pi
        re[:, lo + hs], im[:, lo + hs] = ar - pr, ai - pi
        hs *= 2
    return re, im


def f32_polyphase(x, taps, M, O, cols):
    """complex64 [M][len(cols)]: the evaluation in float32 steps, as the kernel spells them."""
    h = np.asarray(taps, dtype=np.float32)
    T, D, P = len(h), M // O, len(h) // M
    cols = np.asarray(cols)
    pad = np.concatenate([np.zeros(T, dtype=np.complex64), np.asarray(x, dtype=np.complex64)])
    p = np.arange(M)
    ur = np.zeros((len(cols), M), dtype=np.float32)
    ui = np.zeros((len(cols), M), dtype=np.float32)
    for q in range(P):
        s = pad[T + cols[:, None] * D - p[None, :] - M * q]
        ur = _fma(h[p + M * q][None, :], s.real.astype(np.float32), ur)
        ui = _fma(h[p + M * q][None, :], s.imag.astype(np.float32), ui)
    zr, zi = f32_transform(ur, ui, M)
    k = (np.outer(cols, p) * (4 // O)) % 4                          # quarter turns of (-i)
    yr = np.choose(k, [zr, zi, -zr, -zi])
    yi = np.choose(k, [zi, -zr, -zi, zr])
    return (yr + 1j * yi).astype(np.complex64).T


# ------------------------------------------------------------------------------------------ the integer model
def int_channel(iq, scale, taps, M, O, c, cols):
    """complex64 [len(cols)]: channel c in (0, M/4, M/2, 3M/4) in exact integer arithmetic; iq int64 [n][2], taps integers."""
    assert (4 * c) % M == 0
    step = 4 * c // M                                              # quarter turns of -i per input sample
    h = np.asarray(taps, dtype=np.int64)
    T, D = len(h), M // O
    n = np.arange(len(iq))
    q = (step * n) % 4
    i, r = iq[:, 0], iq[:, 1]
    re = np.choose(q, [i, r, -i, -r])
    im = np.choose(q, [r, -i, -r, i])
    pre = np.concatenate([np.zeros(T, dtype=np.int64), re])
    pim = np.concatenate([np.zeros(T, dtype=np.int64), im])
    idx = T + np.asarray(cols)[:, None] * D - np.arange(T)[None, :]
    yr, yi = pre[idx] @ h, pim[idx] @ h
    return ((yr + 1j * yi) / scale).astype(np.complex64)


def bound(taps, max_abs_x, M, P):
    """(P + 4 log2 M + 16) 2^-24 sum|h| max|x|: P units for the chain of a branch sum, 4 per radix-2 level (a butterfly with
    one complex multiply is below 4 units of the sum of magnitudes that enters it), 16 for unpack and margin as in
    ddc_model.bound."""
    h = np.asarray(taps, dtype=np.float64)
    return (P + 4 * (M.bit_length() - 1) + 16) * 2.0 ** -24 * np.abs(h).sum() * max_abs_x


def plan(M, O, P):
    """(W, pitch, lds_bytes, threads) of the kernel's plan, the rule of DESIGN 4.16: the largest power of two W <= min(256, 8192 / M) whose
    LDS (twiddles, W rows of the workspace, the span) stays at 80 KiB if that is 16 columns or all that M allows, else the largest
    that stays at 160 KiB; 256 threads where four workgroups share a CU's LDS, 512 where two do, 1024 where one has it alone."""
    D, T, wmax = M // O, M * P, min(256, 8192 // M)

    def lds(W):
        pitch = M + 1 if W > 1 else M
        return 8 * (max(M // 2, 2) + ((W * pitch + 1) & ~1) + (W - 1) * D + T)
    cands = [wmax >> s for s in range(wmax.bit_length())]
    W = next((c for c in cands if lds(c) <= 80 * 1024 and c >= min(16, wmax)), None)
    if W is None:
        W = next(c for c in cands if lds(c) <= 160 * 1024)
    return W, (M + 1 if W > 1 else M), lds(W), max(M, 256 if lds(W) <= 40 * 1024 else 512 if lds(W) <= 80 * 1024 else 1024)
