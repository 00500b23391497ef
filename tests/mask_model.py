"""The float32 model of the frequency-mask trigger (include/ksa_mask.h, "Semantics"), numpy only: the reference every mask
test compares against, exactly.  Per bin: nan = x != x, over = x > upper with excess x - upper, under = x < lower with
excess lower - x, each one np.float32 subtraction.  Per row: the three counts, the peak = the largest excess with the lowest
bin among equals, an event when nover + nunder >= min_bins or nnan > 0.  The event list keeps the first `capacity` events in
ascending row order; the total counts them all."""
import numpy as np

EVENT_DTYPE = np.dtype([("row", "<i8"), ("nover", "<i4"), ("nunder", "<i4"), ("nnan", "<i4"), ("peak_bin", "<i4"),
                        ("peak_excess", "<f4"), ("peak_kind", "<i4")])


def lines(nbins, upper, lower=None):
    up = np.broadcast_to(np.asarray(upper, dtype=np.float32), (nbins,)).copy()
    lo = np.full(nbins, -np.inf, dtype=np.float32) if lower is None else \
        np.broadcast_to(np.asarray(lower, dtype=np.float32), (nbins,)).copy()
    assert not np.isnan(up).any() and not np.isnan(lo).any() and np.all(lo <= up)
    return up, lo


def check(rows, upper, lower=None, min_bins=1, capacity=4096, row_base=0):
    """rows float32 [k][nbins] -> dict: hits int64 [3][nbins], per-row nover / nunder / nnan / peak_bin / peak_excess /
    peak_kind / event, events (EVENT_DTYPE, at most `capacity`, ascending rows from row_base) and total."""
    rows = np.asarray(rows, dtype=np.float32)
    rows = rows.reshape(-1, rows.shape[-1])
    k, nbins = rows.shape
    up, lo = lines(nbins, upper, lower)
    with np.errstate(invalid="ignore", over="ignore"):
        nan = rows != rows
        over = rows > up
        under = rows < lo
        assert not (over & under).any()
        excess = np.where(over, rows - up, np.where(under, lo - rows, np.float32(-1.0))).astype(np.float32)
    assert not np.isnan(excess).any()                            # never inf - inf
    hits = np.stack([over.sum(axis=0), under.sum(axis=0), nan.sum(axis=0)]).astype(np.int64)
    nover, nunder, nnan = (m.sum(axis=1).astype(np.int32) for m in (over, under, nan))
    crossed = (nover + nunder) > 0
    peak_bin = np.where(crossed, np.argmax(excess, axis=1), -1).astype(np.int32) if k else np.zeros(0, np.int32)   # argmax: the first
    at = np.maximum(peak_bin, 0)
    idx = np.arange(k)
    peak_excess = np.where(crossed, excess[idx, at], np.float32(0)).astype(np.float32)
    peak_kind = np.where(crossed, np.where(under[idx, at], 1, 0), -1).astype(np.int32)
    event = ((nover + nunder) >= min_bins) | (nnan > 0)
    which = np.flatnonzero(event)
    ev = np.zeros(min(len(which), capacity), dtype=EVENT_DTYPE)
    keep = which[:capacity]
    ev["row"] = keep + row_base
    for name, arr in (("nover", nover), ("nunder", nunder), ("nnan", nnan), ("peak_bin", peak_bin),
                      ("peak_excess", peak_excess), ("peak_kind", peak_kind)):
        ev[name] = arr[keep]
    return dict(hits=hits, nover=nover, nunder=nunder, nnan=nnan, peak_bin=peak_bin, peak_excess=peak_excess,
                peak_kind=peak_kind, event=event, events=ev, total=int(len(which)))


def learn_mask(rows, margin_db):
    """np.fmax.reduce(rows, axis=0) + np.float32(margin_db) in float32; a bin that is NaN in every row becomes +inf."""
    r = np.asarray(rows, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        up = (np.fmax.reduce(r, axis=0) + np.float32(margin_db)).astype(np.float32)
    up[np.isnan(up)] = np.inf
    return up


def events_equal(a, b):
    """Field by field, exactly (peak_excess by its bits, so that +inf and every rounding count)."""
    if a.shape != b.shape:
        return False
    return all(np.array_equal(a[n].view(np.int32) if n == "peak_excess" else a[n],
                              b[n].view(np.int32) if n == "peak_excess" else b[n]) for n in EVENT_DTYPE.names)
