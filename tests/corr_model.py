"""numpy model of include/ksa_corr.h, the oracle of the correlator's tests (the reference has no counterpart).

Definition: r_q[n] = sum_k conj(c_q[k]) x[n+k], e[n] = sum_k |x[n+k]|^2, Ec[q] = sum_k |c_q[k]|^2,
rho_q[n] = |r_q[n]|^2 / (e[n] Ec[q]) where e[n] Ec[q] > 0 and e[n] >= min_energy, else 0.  Three forms: the float64 definition;
a float32 emulation of the chains as the header orders them (two fused multiply-adds per k and chain); and an exact model for
small-integer samples and templates in {+-1, +-j}, where every sum is an integer below 2^24 and the only rounding left is the
one correctly rounded division.

Bounds of the float test (u = 2^-24), derived, not measured:
- A part of r is a chain of 2K fused multiply-adds: every partial sum is rounded once, the products not at all, so the error
  is at most gamma_2K sum|terms| with gamma_2K ~ 2K u; two further units cover the higher-order terms (2K u <= 2^-11) and the
  comparison of a float32 value with the float64 reference.  Per part:
      B_re = (2K + 2) u sum_k (|xr||cr| + |xi||ci|),    B_im = (2K + 2) u sum_k (|xr||ci| + |xi||cr|).
- e is such a chain of non-negative terms: relative error at most (2K + 2) u.
- rho_hat = (p + dp) / (den (1 + eta)) (1 + delta) with |delta| <= u (the division),
      |eta| <= (2K + 2) u + 3 u      (e, the rounding of Ec to float32, the rounding of e * Ec, their cross terms),
      |dp|  <= (2|re| B_re + B_re^2 + 2|im| B_im + B_im^2)(1 + 2u) + 2u p      (the errors of re and im, the roundings of im*im
                                                                                and of the fused multiply-add),
  hence |rho_hat - rho| <= (rho (|eta| + u) + |dp| (1 + u) / den) / (1 - |eta|), and 1 / (1 - |eta|) <= 1.001 for K <= 4096."""
import numpy as np

from resamp_model import _fma32

U = 2.0 ** -24
EVENT_DTYPE = np.dtype([("pos", "<i8"), ("block", "<i4"), ("templ", "<i4"), ("metric", "<f4"), ("metric_prev", "<f4"),
                        ("metric_next", "<f4"), ("re", "<f4"), ("im", "<f4")])


def lags_after(seen, K):
    return max(0, int(seen) - K + 1)


def out_count(seen, n, K):
    """Lags a stream call of n samples completes after `seen` samples."""
    return lags_after(seen + n, K) - lags_after(seen, K)


def _templates(c):
    c = np.asarray(c)
    return c[None, :] if c.ndim == 1 else c


# -- float64 definition ------------------------------------------------------------------------------------------------------
def energy(x, K):
    """float64 [lags]: the window energies, each summed on its own (no running sum)."""
    p = np.abs(np.asarray(x, dtype=np.complex128)) ** 2
    return np.lib.stride_tricks.sliding_window_view(p, K).sum(axis=1) if len(p) >= K else np.zeros(0)


def definition(x, c, min_energy=0.0):
    """(rho float64 [Q][lags], r complex128 [Q][lags]) of the samples x against the templates c [Q][K] (float32 values)."""
    x = np.asarray(x, dtype=np.complex128)
    c = _templates(c).astype(np.complex128)
    Q, K = c.shape
    n = lags_after(len(x), K)
    r = np.zeros((Q, n), dtype=np.complex128)
    if n:
        for q in range(Q):
            r[q] = np.correlate(x, c[q], "valid")                # sum_k x[n+k] conj(c[k])
    e = energy(x, K)
    ec = (np.abs(c) ** 2).sum(axis=1)
    den = e[None, :] * ec[:, None]
    ok = (den > 0) & (e[None, :] >= min_energy)
    rho = np.where(ok, np.abs(r) ** 2 / np.where(ok, den, 1.0), 0.0)
    return rho, r


def bounds(x, c, rho, r):
    """(B_rho [Q][lags], B_re, B_im) of the module's docstring, from the float64 definition's rho and r."""
    x = np.asarray(x, dtype=np.complex128)
    c = _templates(c).astype(np.complex128)
    Q, K = c.shape
    axr, axi = np.abs(x.real), np.abs(x.imag)
    g = (2 * K + 2) * U
    b_re, b_im = np.zeros(rho.shape), np.zeros(rho.shape)
    for q in range(Q):
        acr, aci = np.abs(c[q].real), np.abs(c[q].imag)
        b_re[q] = g * (np.correlate(axr, acr, "valid") + np.correlate(axi, aci, "valid"))
        b_im[q] = g * (np.correlate(axr, aci, "valid") + np.correlate(axi, acr, "valid"))
    e = energy(x, K)
    den = e[None, :] * (np.abs(c) ** 2).sum(axis=1)[:, None]
    p = np.abs(r) ** 2
    dp = (2 * np.abs(r.real) * b_re + b_re ** 2 + 2 * np.abs(r.imag) * b_im + b_im ** 2) * (1 + 2 * U) + 2 * U * p
    eta = g + 3 * U
    with np.errstate(divide="ignore", invalid="ignore"):
        b_rho = np.where(den > 0, (rho * (eta + U) + dp * (1 + U) / den) / (1 - eta), 0.0)
    return b_rho, b_re, b_im


def worst_ratios(got_rho, got_r, x, c):
    """(worst |rho error| / bound, worst |r part error| / bound) against the float64 definition; values whose bound is zero
    must be exact."""
    rho, r = definition(x, c)
    b_rho, b_re, b_im = bounds(x, c, rho, r)
    worst = []
    for pairs in ([(got_rho, rho, b_rho)], [(got_r.real, r.real, b_re), (got_r.imag, r.imag, b_im)]):
        w = 0.0
        for g, want, b in pairs:
            err = np.abs(np.asarray(g, dtype=np.float64) - want)
            assert np.all(err[b == 0] == 0)
            if np.any(b > 0):
                w = max(w, float(np.max(err[b > 0] / b[b > 0])))
        worst.append(w)
    return tuple(worst)


# -- float32 emulation --------------------------------------------------------------------------------------------------------
def ec32(c):
    """float32 [Q]: the template energies, summed in float64 and rounded once."""
    c = _templates(c).astype(np.complex64)
    return (c.real.astype(np.float64) ** 2 + c.imag.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)


def f32_chain(x, c, min_energy=0.0):
    """(rho float32 [Q][lags], r complex64 [Q][lags]) by the header's chains: k ascending, the real part's term before the
    imaginary part's, every accumulator from +0, then p = fmaf(re, re, im * im), den = e * Ec, rho = p / den."""
    x = np.asarray(x, dtype=np.complex64)
    c = _templates(c).astype(np.complex64)
    Q, K = c.shape
    n = lags_after(len(x), K)
    xr, xi = x.real.astype(np.float32), x.imag.astype(np.float32)
    cr, ci = c.real.astype(np.float32), c.imag.astype(np.float32)
    re, im = np.zeros((Q, n), dtype=np.float32), np.zeros((Q, n), dtype=np.float32)
    e = np.zeros(n, dtype=np.float32)
    for k in range(K if n else 0):
        a, b = xr[k:k + n], xi[k:k + n]
        for q in range(Q):
            re[q] = _fma32(a, np.broadcast_to(cr[q, k], a.shape), re[q])
            re[q] = _fma32(b, np.broadcast_to(ci[q, k], a.shape), re[q])
            im[q] = _fma32(a, np.broadcast_to(-ci[q, k], a.shape), im[q])
            im[q] = _fma32(b, np.broadcast_to(cr[q, k], a.shape), im[q])
        e = _fma32(a, a, e)
        e = _fma32(b, b, e)
    p = _fma32(re, re, im * im)
    den = e[None, :] * ec32(c)[:, None]
    ok = (den > 0) & (e[None, :] >= np.float32(min_energy))
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = np.where(ok, p / np.where(ok, den, np.float32(1)), np.float32(0)).astype(np.float32)
    return rho, (re + 1j * im).astype(np.complex64)


# -- exact: samples with integer parts in [-4, 4], template values in {1, -1, j, -j}, K <= 256 ----------------------------------
def exact_samples(rng, n):
    return (rng.integers(-4, 5, n) + 1j * rng.integers(-4, 5, n)).astype(np.complex64)


def exact_templates(rng, Q, K):
    return np.array([1, -1, 1j, -1j], dtype=np.complex64)[rng.integers(0, 4, (Q, K))]


def exact_model(x, c, min_energy=0.0):
    """Bit-exact (rho float32, r complex64): int64 sums, then one float32 division of two integers below 2^24."""
    c = _templates(c)
    Q, K = c.shape                                               # K <= 256 for exact_samples; beyond, sparser samples: the asserts below
    xr, xi = np.rint(np.real(x)).astype(np.int64), np.rint(np.imag(x)).astype(np.int64)
    cr, ci = np.rint(c.real).astype(np.int64), np.rint(c.imag).astype(np.int64)
    assert np.abs(xr).max(initial=0) <= 4 and np.abs(xi).max(initial=0) <= 4 and np.all(np.abs(cr) + np.abs(ci) == 1)
    n = lags_after(len(xr), K)
    re, im = np.zeros((Q, n), dtype=np.int64), np.zeros((Q, n), dtype=np.int64)
    e = np.zeros(n, dtype=np.int64)
    for k in range(K if n else 0):
        a, b = xr[k:k + n], xi[k:k + n]
        re += a[None, :] * cr[:, k, None] + b[None, :] * ci[:, k, None]
        im += b[None, :] * cr[:, k, None] - a[None, :] * ci[:, k, None]
        e += a * a + b * b
    p = re * re + im * im
    den = e[None, :] * np.full((Q, 1), K, dtype=np.int64)
    assert p.max(initial=0) < 2 ** 24 and den.max(initial=0) < 2 ** 24
    ok = (den > 0) & (e[None, :] >= min_energy)
    rho = np.where(ok, p.astype(np.float32) / np.where(ok, den, 1).astype(np.float32), np.float32(0)).astype(np.float32)
    return rho, (re + 1j * im).astype(np.complex64)


# -- peaks and records ----------------------------------------------------------------------------------------------------------
def peaks(rho, threshold, G):
    """The lags n of one row with rho[n] >= threshold, no rho[j] >= rho[n] in [n-G, n) and no rho[j] > rho[n] in (n, n+G]."""
    rho = np.asarray(rho)
    out = []
    for n in np.flatnonzero(rho >= np.float32(threshold)):
        v = rho[n]
        if np.any(rho[max(0, n - G):n] >= v) or np.any(rho[n + 1:n + G + 1] > v):
            continue
        out.append(int(n))
    return out


def records(rho, r, threshold, G, block=-1, pos_base=0, first=0, last=None):
    """The events of one stream or block in (pos, templ) order: rho float32 [Q][lags], r complex64 [Q][lags]; only the peaks at
    lags [first, last) are listed (the decided ones), the neighbourhood is all of rho."""
    Q, n = rho.shape
    last = n if last is None else last
    found = sorted((p, q) for q in range(Q) for p in peaks(rho[q], threshold, G) if first <= p < last)
    ev = np.zeros(len(found), dtype=EVENT_DTYPE)
    for i, (p, q) in enumerate(found):
        ev[i] = (pos_base + p, block, q, rho[q, p], rho[q, p - 1] if p > 0 else 0, rho[q, p + 1] if p + 1 < n else 0,
                 r[q, p].real, r[q, p].imag)
    return ev


def block_records(rho, r, threshold, G):
    """The events of the block form: rho [nblocks][Q][lags], blocks in order."""
    parts = [records(rho[b], r[b], threshold, G, block=b) for b in range(len(rho))]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=EVENT_DTYPE)


def refine(ev):
    """The three-point parabola, in float64; pos where it is degenerate."""
    pos = ev["pos"].astype(np.float64)
    a, b, c = (ev[k].astype(np.float64) for k in ("metric_prev", "metric", "metric_next"))
    den = a - 2 * b + c
    d = np.where(den < 0, 0.5 * (a - c) / np.where(den < 0, den, 1.0), 0.0)
    return pos + np.clip(d, -0.5, 0.5)
