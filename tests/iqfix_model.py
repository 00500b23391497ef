"""The DC-offset and IQ-imbalance corrector of include/ksa_iqfix.h in numpy: float32 arrays for every per-sample step, np.rint
and then int64 for the five quantities, Python float64 (one rounding per operation, in the header's order) for the solve.
Every comparison with the GPU is np.array_equal: no tolerance exists in this feature.  ddc_model.unpack works in float64 and
does not fit; the unpack here is the header's, step by step in float32."""
import math

import numpy as np

UNIT = 1 << 30
MAX_COUNT = 1 << 30
MODE_DC, MODE_IQ = 1, 2
FLAG_DEGENERATE, FLAG_EMPTY = 1, 2
IDENTITY = (0.0, 0.0, 0.0, 1.0)
F32 = np.float32
FORMATS = ("c64", "u8", "s8", "s16")
DTYPES = {"c64": np.complex64, "u8": np.uint8, "s8": np.int8, "s16": np.int16}


def unpack(raw, fmt="c64", u8_offset=127.5, u8_scale=127.5):
    """(xr, xi) float32 of raw samples: complex64 [n], or an integer array [n][2]."""
    if fmt == "c64":
        x = np.ascontiguousarray(raw, dtype=np.complex64).reshape(-1)
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
    return np.rint(v.astype(F32) * F32(UNIT)).astype(np.int64)       # the product is exact; rint rounds ties to even


def quantities(xr, xi):
    """(aI, aQ, cII, cQQ, cIQ), int64 [n] each."""
    xr, xi = np.asarray(xr, dtype=F32), np.asarray(xi, dtype=F32)
    four = F32(4.0)
    clamp = lambda v: np.maximum(np.minimum(v, four), -four)
    with np.errstate(over="ignore"):                                 # a product beyond float32 is an infinity, which saturates
        return (_to_int(clamp(xr)), _to_int(clamp(xi)), _to_int(np.minimum(xr * xr, four)), _to_int(np.minimum(xi * xi, four)),
                _to_int(clamp(xr * xi)))


def stats(xr, xi):
    """int64 [6]: the five sums and the count, as Python-exact integers in an int64 array."""
    q = quantities(xr, xi)
    return np.array([int(v.sum(dtype=np.int64)) for v in q] + [len(q[0])], dtype=np.int64)


def solve(sums, mode):
    """dict(dc_i, dc_q, c, d, flags, mode, count) from the six words; the four coefficients are float32 values."""
    s = [int(v) for v in sums]
    out = dict(dc_i=F32(0), dc_q=F32(0), c=F32(0), d=F32(1), flags=0, mode=int(mode), count=s[5])
    if s[5] == 0:
        out["flags"] = FLAG_EMPTY
        return out
    u = float(s[5]) * 1073741824.0
    mI = float(s[0]) / u
    mQ = float(s[1]) / u
    vII = float(s[2]) / u - mI * mI
    vQQ = float(s[3]) / u - mQ * mQ
    vIQ = float(s[4]) / u - mI * mQ
    if mode & MODE_DC:
        out["dc_i"], out["dc_q"] = F32(mI), F32(mQ)
    if mode & MODE_IQ:
        valid = False
        if vII > 0.0:
            r = vIQ / vII
            w = vQQ - r * vIQ
            if w > 0.0:
                ratio = vII / w
                if 2.0 ** -8 <= ratio <= 2.0 ** 8:
                    d = math.sqrt(ratio)
                    c = -(d * r)
                    out["c"], out["d"] = F32(c), F32(d)
                    valid = True
        if not valid:
            out["flags"] |= FLAG_DEGENERATE
    return out


def coeffs_of(sol):
    """(dc_i, dc_q, c, d) of a solve's dict."""
    return sol["dc_i"], sol["dc_q"], sol["c"], sol["d"]


def apply(xr, xi, coeffs=IDENTITY):
    """complex64 [n]: the four float32 operations of the header, each rounded on its own."""
    dc_i, dc_q, c, d = (F32(v) for v in coeffs)
    xr, xi = np.asarray(xr, dtype=F32), np.asarray(xi, dtype=F32)
    ui = xr - dc_i
    uq = xi - dc_q
    yq = (c * ui).astype(F32) + (d * uq).astype(F32)
    out = np.empty(len(xr), dtype=np.complex64)
    out.real, out.imag = ui, yq
    return out


def imbalance_of(c, d):
    """(gain error in dB, phase error in degrees): gain = 1 / hypot(c, d), phase = atan2(-c, d)."""
    c, d = float(c), float(d)
    return 20.0 * math.log10(1.0 / math.hypot(c, d)), math.degrees(math.atan2(-c, d))


def impaired_capture(n, seed=20261020, amplitude=0.3, sigma=0.01, gain_db=1.0, phase_deg=5.0, dc=(0.05, -0.03)):
    """int16 [n][2]: a tone of `amplitude` at bin n/8 plus complex noise of `sigma` per component, through a receiver with a
    gain error of gain_db and a phase error of phase_deg on Q and a DC offset, quantised to int16."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    z = amplitude * np.exp(2j * np.pi * (n // 8) * t / n) + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    g, phi = 10.0 ** (gain_db / 20.0), np.radians(phase_deg)
    i = z.real + dc[0]
    q = g * (z.real * np.sin(phi) + z.imag * np.cos(phi)) + dc[1]
    return np.stack([np.rint(i * 32768.0), np.rint(q * 32768.0)], axis=-1).clip(-32768, 32767).astype(np.int16)


def rejections(y):
    """(image rejection, DC rejection) in dB of complex samples [n] holding a tone at bin n/8: the power over 5 bins around
    the tone against that over 5 bins around its image at -n/8, and against that around bin 0, under a hanning window."""
    n = len(y)
    p = np.abs(np.fft.fft(np.asarray(y, dtype=np.complex128) * np.hanning(n))) ** 2
    band = lambda k: sum(p[(k + j) % n] for j in range(-2, 3))
    tone = band(n // 8)
    return 10 * np.log10(tone / band(-(n // 8))), 10 * np.log10(tone / band(0))
