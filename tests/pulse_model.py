"""The pulse detector of include/ksa_pulse.h in numpy: float32 arrays for p, re and im, np.rint and then int64, np.cumsum for
S, and a plain Python loop for the hysteresis and the runs.  Every comparison with the GPU is np.array_equal, field by field:
no tolerance exists in this feature."""
import numpy as np

UNIT = 1 << 30
FLAG_OPEN_END = 1
EVENT_DTYPE = np.dtype([("start", "<i8"), ("len", "<i8"), ("energy", "<i8"), ("peak", "<i8"), ("peak_pos", "<i8"), ("dre", "<i8"),
                        ("dim", "<i8"), ("block", "<i4"), ("flags", "<i4")])
F32 = np.float32


def unpack(raw, fmt="c64", u8_offset=127.5, u8_scale=127.5):
    """(xr, xi) float32 of raw samples: complex64 [n], or an integer array [n][2]."""
    if fmt == "c64":
        x = np.ascontiguousarray(raw, dtype=np.complex64)
        return x.real.astype(F32), x.imag.astype(F32)
    a = np.asarray(raw).reshape(-1, 2)
    if fmt == "u8":
        inv = F32(1.0) / F32(u8_scale)
        v = (a.astype(F32) - F32(u8_offset)) * inv
    elif fmt == "s8":
        v = a.astype(F32) * F32(2.0 ** -7)
    else:
        v = a.astype(F32) * F32(2.0 ** -15)
    return np.ascontiguousarray(v[:, 0], dtype=F32), np.ascontiguousarray(v[:, 1], dtype=F32)


def _to_int(v):
    return np.rint(v.astype(F32) * F32(UNIT)).astype(np.int64)


def quantities(xr, xi):
    """(q, dre, dim) int64 [n]; dre and dim of sample 0 pair it with (0, 0) and are never used."""
    xr, xi = np.asarray(xr, dtype=F32), np.asarray(xi, dtype=F32)
    p = xr * xr + xi * xi                                        # each operation rounds to float32
    q = _to_int(np.minimum(p, F32(4.0)))
    yr, yi = np.concatenate([[F32(0)], xr[:-1]]).astype(F32), np.concatenate([[F32(0)], xi[:-1]]).astype(F32)
    re = xr * yr + xi * yi
    im = xi * yr - xr * yi
    clamp = lambda v: np.minimum(np.maximum(v, F32(-4.0)), F32(4.0))
    return q, _to_int(clamp(re)), _to_int(clamp(im))


def envelope(q, W):
    """S[n] = q[n-W+1] + ... + q[n], q being 0 before the start."""
    c = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(q, dtype=np.int64)])
    n = np.arange(len(q))
    return c[n + 1] - c[np.maximum(n + 1 - W, 0)]


def thresholds(on_power, off_power, W):
    """(thr_on, thr_off) as the library forms them: float32 powers, exact products in float64, llrint."""
    on = int(np.rint(np.float64(F32(on_power)) * UNIT * W))
    off = int(np.rint(np.float64(F32(off_power)) * UNIT * W))
    return on, off


def active_of(S, thr_on, thr_off):
    act = np.zeros(len(S), dtype=bool)
    state = False
    for n, s in enumerate(S.tolist()):
        if s >= thr_on:
            state = True
        elif s < thr_off:
            state = False
        act[n] = state
    return act


def runs_of(q, dre, dim, S, act, min_len, block=-1, flushed=True):
    """Records of the maximal runs of act, in order; the run still active at the end only when flushed, with the flag."""
    out = []
    n, N = 0, len(act)
    while n < N:
        if not act[n]:
            n += 1
            continue
        a = n
        while n < N and act[n]:
            n += 1
        open_end = n == N
        if open_end and not flushed:
            break
        if n - a < min_len:
            continue
        seg = S[a:n]
        out.append((a, n - a, int(q[a:n].sum()), int(seg.max()), a + int(np.argmax(seg)), int(dre[a + 1:n].sum()), int(dim[a + 1:n].sum()),
                    block, FLAG_OPEN_END if open_end else 0))
    return np.array(out, dtype=EVENT_DTYPE) if out else np.zeros(0, dtype=EVENT_DTYPE)


def detect(raw, W, on_power, off_power, min_len=1, fmt="c64", u8_offset=127.5, u8_scale=127.5, block=-1, flushed=True):
    """(S int64 [n], records, active flags [n]) of one stream or block from its start."""
    xr, xi = unpack(raw, fmt, u8_offset, u8_scale)
    q, dre, dim = quantities(xr, xi)
    S = envelope(q, W)
    on, off = thresholds(on_power, off_power, W)
    act = active_of(S, on, off)
    return S, runs_of(q, dre, dim, S, act, min_len, block, flushed), act


def describe(ev, W, sampling_rate, full_size=0):
    """The .npz fields of a pulse list."""
    fs = float(sampling_rate)
    block = np.maximum(ev["block"].astype(np.float64), 0.0)
    ln = ev["len"].astype(np.float64)
    return {"toa_s": (block * full_size + ev["start"]) / fs, "width_s": ln / fs,
            "mean_dbfs": 10 * np.log10(ev["energy"] / UNIT / ln), "peak_dbfs": 10 * np.log10(ev["peak"] / UNIT / W),
            "freq_hz": np.arctan2(ev["dim"].astype(np.float64), ev["dre"].astype(np.float64)) / (2 * np.pi) * fs}
