"""Float64 model of libksa_measure (include/ksa_measure.h) -- TEST INFRASTRUCTURE: numpy float64 with math.fsum for the sums
and the header's rules taken literally.  Beside every record the model returns the task's margin: how close the data come to
flipping one of the exact fields, so that a test can assert its input is decidable before it asserts equality."""
import math

import numpy as np

RESULT_DTYPE = np.dtype([("row", "<i8"), ("bin_lo", "<i4"), ("bin_hi", "<i4"), ("nvalid", "<i4"), ("flags", "<i4"),
                         ("power", "<f8"), ("m1", "<f8"), ("m2", "<f8"), ("peak_bin", "<i4"), ("peak_db", "<f4"),
                         ("obw_lo", "<i4"), ("obw_hi", "<i4"), ("xdb_lo", "<i4"), ("xdb_hi", "<i4"), ("power_db", "<f4"),
                         ("reserved", "<i4")])
OFFSETS = {"row": 0, "bin_lo": 8, "bin_hi": 12, "nvalid": 16, "flags": 20, "power": 24, "m1": 32, "m2": 40, "peak_bin": 48,
           "peak_db": 52, "obw_lo": 56, "obw_hi": 60, "xdb_lo": 64, "xdb_hi": 68, "power_db": 72, "reserved": 76}
FLAG_MEASURED, FLAG_CLIPPED, FLAG_INVALID = 1, 2, 4
WAVE_MAX_BINS = 256
EXACT = ("row", "bin_lo", "bin_hi", "nvalid", "flags", "peak_bin", "obw_lo", "obw_hi", "xdb_lo", "xdb_hi", "reserved")
SUMS = ("power", "m1", "m2")
SUM_RTOL = 1e-12            # (b - a + 1) * 2^-53 at the widest window of the tests, one ulp of the float64 10^x, headroom
MIN_MARGIN = 1e-9

# every kernel of the library's gfx950 code object and the GPU test that launches it
KERNELS = {
    "ksa::measure::measure_kernel<false, false>": "tests/test_gpu_measure.py::test_bands_match_the_model",
    "ksa::measure::measure_kernel<false, true>": "tests/test_gpu_measure.py::test_bands_match_the_model",
    "ksa::measure::measure_kernel<true, false>": "tests/test_gpu_measure.py::test_bands_match_the_model",
    "ksa::measure::measure_kernel<true, true>": "tests/test_gpu_measure.py::test_bands_match_the_model",
}


def powers(x):
    """(valid [n] bool, xc [n] float32, p [n] float64) of float32 dB values."""
    x = np.asarray(x, dtype=np.float32)
    valid = ~np.isnan(x) & (x != -np.inf)
    with np.errstate(invalid="ignore"):
        xc = np.minimum(np.maximum(x, np.float32(-500)), np.float32(500)).astype(np.float32)
    xc = np.where(valid, xc, np.float32(0)).astype(np.float32)
    p = np.where(valid, np.power(10.0, xc.astype(np.float64) / 10.0), 0.0)
    return valid, xc, p


def measure(row, a, b, occupied=0.99, xdb=3.0, row_id=0, flags=FLAG_MEASURED):
    """(record, margin) of the window [a, b] of one float32 row.  margin = the smallest of |partial sum - tail| / power over
    the two partial sums on either side of each OBW edge and |xc - threshold| over the bins next to each x-dB edge (inf where
    there is no such neighbour)."""
    row = np.asarray(row, dtype=np.float32)
    assert 0 <= a <= b < len(row)
    x = row[a:b + 1]
    valid, xc, p = powers(x)
    n = int(b - a + 1)
    r = np.zeros((), dtype=RESULT_DTYPE)
    r["row"], r["bin_lo"], r["bin_hi"], r["nvalid"] = row_id, a, b, int(valid.sum())
    r["flags"] = flags | (FLAG_INVALID if valid.sum() < n else 0)
    k = np.arange(n, dtype=np.float64)
    power = math.fsum(p)
    r["power"], r["m1"], r["m2"] = power, math.fsum(p * k), math.fsum(p * k * k)
    if not valid.any():
        r["power_db"], r["peak_bin"], r["peak_db"] = -np.inf, -1, np.nan
        r["obw_lo"] = r["obw_hi"] = r["xdb_lo"] = r["xdb_hi"] = -1
        return r, math.inf
    r["power_db"] = np.float32(10.0 * math.log10(power))
    best = xc[valid].max()
    pk = int(np.flatnonzero(valid & (xc == best))[0])          # +0 == -0: the lowest bin among equals
    r["peak_bin"], r["peak_db"] = a + pk, x[pk]
    beta = float(np.float32(occupied))
    tail = (1.0 - beta) / 2.0 * power
    wide = p.astype(np.longdouble)      # the running sums in extended precision: n * 2^-64 is far inside every margin asked for
    prefix = np.cumsum(wide)                                   # sum over [a, a+i]
    suffix = np.cumsum(wide[::-1])[::-1]                       # sum over [a+i, b]
    lo = int(np.flatnonzero(prefix > tail)[0])
    hi = int(np.flatnonzero(suffix > tail)[-1])
    r["obw_lo"], r["obw_hi"] = a + lo, a + hi
    margin = min(abs(prefix[lo] - tail), abs(suffix[hi] - tail)) / power
    if lo > 0:
        margin = min(margin, abs(prefix[lo - 1] - tail) / power)
    if hi < n - 1:
        margin = min(margin, abs(suffix[hi + 1] - tail) / power)
    thr = np.float32(best - np.float32(xdb))
    above = np.flatnonzero(valid & (xc >= thr))
    r["xdb_lo"], r["xdb_hi"] = a + above[0], a + above[-1]
    near = [i for i in (above[0] - 1, above[0], above[-1], above[-1] + 1) if 0 <= i < n and valid[i] and i != pk]
    for i in near:
        margin = min(margin, abs(float(xc[i]) - float(thr)))
    return r, float(margin)


def measure_spans(rows, spans, total, capacity, occupied=0.99, xdb=3.0, margin=0, row_base=0, first=0, span_capacity=None,
                  before=None):
    """(results [capacity], margins [capacity]) after one spans call over rows [nrows][nbins]: spans is a structured array
    whose records begin with row, bin_lo, bin_hi; `before` are the results as they were (default: zero)."""
    rows = np.asarray(rows, dtype=np.float32)
    nrows, nbins = rows.shape
    out = np.zeros(capacity, dtype=RESULT_DTYPE) if before is None else np.array(before)
    margins = np.full(capacity, math.inf)
    lim = min(int(total), len(spans) if span_capacity is None else int(span_capacity), capacity)
    for i in range(first, lim):
        s = spans[i]
        row, lo, hi = int(s["row"]), int(s["bin_lo"]), int(s["bin_hi"])
        if not row_base <= row < row_base + nrows or lo < 0 or hi >= nbins or lo > hi:
            continue
        a, b = max(lo - margin, 0), min(hi + margin, nbins - 1)
        clipped = FLAG_CLIPPED if (a != lo - margin or b != hi + margin) else 0
        out[i], margins[i] = measure(rows[row - row_base], a, b, occupied, xdb, row, FLAG_MEASURED | clipped)
    return out, margins


def measure_bands(rows, bands, capacity, occupied=0.99, xdb=3.0, row_base=0, first_slot=0, before=None):
    """(results [capacity], margins [capacity]) after one bands call."""
    rows = np.asarray(rows, dtype=np.float32)
    out = np.zeros(capacity, dtype=RESULT_DTYPE) if before is None else np.array(before)
    margins = np.full(capacity, math.inf)
    nb = len(bands)
    for r in range(len(rows)):
        for j, (lo, hi) in enumerate(bands):
            i = first_slot + r * nb + j
            out[i], margins[i] = measure(rows[r], int(lo), int(hi), occupied, xdb, row_base + r)
    return out, margins


def ulps32(a, b):
    """Distance in float32 ulps between two float32 values of one sign (equal infinities: 0)."""
    a, b = np.float32(a), np.float32(b)
    if a == b:
        return 0
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def compare(got, want, margins, where=""):
    """Assert that the records `got` are the model's `want`: the integer fields and peak_db exactly -- after asserting that
    the model's margin makes them decidable --, the sums within SUM_RTOL, power_db within 2 float32 ulps."""
    assert len(got) == len(want) == len(margins)
    for i in range(len(want)):
        g, w, tag = got[i], want[i], "%s record %d" % (where, i)
        assert margins[i] >= MIN_MARGIN, (tag, margins[i])
        for f in EXACT:
            assert g[f] == w[f], (tag, f, g[f], w[f], margins[i])
        assert g["peak_db"].tobytes() == w["peak_db"].tobytes() or (np.isnan(g["peak_db"]) and np.isnan(w["peak_db"])
                                                                     and w["peak_bin"] < 0), (tag, g["peak_db"], w["peak_db"])
        for f in SUMS:
            assert abs(g[f] - w[f]) <= SUM_RTOL * abs(w[f]), (tag, f, g[f], w[f])
        assert ulps32(g["power_db"], w["power_db"]) <= 2, (tag, g["power_db"], w["power_db"])
