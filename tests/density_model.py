"""The float32 model of the density histogram (include/ksa_density.h, "Semantics"), numpy only: the reference every density
test compares against, exactly (np.array_equal on int64).  Every step is np.float32 arithmetic in the order the header states:
inv once, one subtraction, one multiplication, NaN first, the two clamps, truncation."""
import numpy as np


def inv_of(levels, lo_db, hi_db):
    """(float)L / (hi_db - lo_db): one float32 subtraction, one float32 division."""
    return np.float32(levels) / (np.float32(hi_db) - np.float32(lo_db))


def level_rows(values, levels, lo_db, hi_db):
    """int64 level index (0..levels; levels = the NaN row) of every float32 value."""
    r = np.asarray(values, dtype=np.float32)
    lo, inv, top = np.float32(lo_db), inv_of(levels, lo_db, hi_db), np.float32(levels)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (r - lo) * inv
        assert t.dtype == np.float32
        nan = np.isnan(r)
        high = ~nan & (t >= top)
        low = ~nan & (t < np.float32(0))
        mid = ~(nan | high | low)
        row = np.zeros(r.shape, dtype=np.int64)
        row[mid] = np.trunc(t[mid]).astype(np.int64)
    row[nan] = levels
    row[high] = levels - 1
    row[low] = 0
    return row


def add_rows(counts, rows, levels, lo_db, hi_db):
    """counts int64 [levels + 1][W] += the histogram of rows float32 [k][nbins]; W must divide nbins.  Returns k."""
    rows = np.asarray(rows, dtype=np.float32)
    rows = rows.reshape(-1, rows.shape[-1])
    width = counts.shape[1]
    nbins = rows.shape[1]
    assert counts.shape[0] == levels + 1 and nbins % width == 0
    g = nbins // width
    lvl = level_rows(rows, levels, lo_db, hi_db)
    col = np.broadcast_to(np.arange(nbins) // g, lvl.shape)
    flat = np.bincount((lvl * width + col).ravel(), minlength=(levels + 1) * width)
    counts += flat.reshape(levels + 1, width).astype(np.int64)
    return rows.shape[0]


def histogram(rows, width, levels, lo_db, hi_db):
    counts = np.zeros((levels + 1, width), dtype=np.int64)
    add_rows(counts, rows, levels, lo_db, hi_db)
    return counts


def decay(counts, num, den):
    """floor(c * num / den) as the header computes it: no product leaves 64 bits."""
    c = np.asarray(counts, dtype=np.int64)
    return (c // den) * num + ((c % den) * num) // den


def edge_values(levels, lo_db, hi_db):
    """float32 values on lo, on hi, on every nominal edge lo + k*step and one float32 ulp either side of each."""
    lo, hi = np.float32(lo_db), np.float32(hi_db)
    k = np.arange(levels + 1, dtype=np.float64)
    e = (np.float64(lo) + k * (np.float64(hi) - np.float64(lo)) / levels).astype(np.float32)
    e[0], e[-1] = lo, hi
    return np.concatenate([e, np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf))]).astype(np.float32)
