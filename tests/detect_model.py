"""The integer model of the CFAR signal detector (include/ksa_detect.h, "Semantics"), numpy only: the reference every detect
test compares against, exactly.  Quantise to 1/64 dB (rint of a float32 product that is exact), prefix sums of q and of `valid`,
window sums as differences of the prefix arrays, the three modes as integer inequalities, opening by min_width, closing by
max_gap, one record per maximal run.  The emission list keeps the first `capacity` records in ascending (row, bin_lo) order; the
total and the hits count them all."""
import numpy as np

EMISSION_DTYPE = np.dtype([("row", "<i8"), ("bin_lo", "<i4"), ("bin_hi", "<i4"), ("peak_bin", "<i4"), ("ndet", "<i4"),
                           ("peak_db", "<f4"), ("floor_db", "<f4")])
MODES = {"ca": 0, "go": 1, "so": 2}
SCALE = np.float32(2.0 ** -6)


def quantise(rows):
    """(q int64, valid bool): q = rint(clip(x, -500, 500) * 64) in float32, 0 where the bin is NaN or -inf."""
    x = np.asarray(rows, dtype=np.float32)
    valid = ~np.isnan(x) & (x != -np.inf)
    safe = np.where(valid, x, np.float32(0))
    prod = np.minimum(np.maximum(safe, np.float32(-500)), np.float32(500)) * np.float32(64)
    assert prod.dtype == np.float32
    q = np.rint(prod).astype(np.int64)
    q[~valid] = 0
    return q, valid


def threshold_q(threshold_db):
    return int(np.rint(np.float32(threshold_db) * np.float32(64)))


def window_sums(q, valid, train, guard):
    """SL, CL, SR, CR int64 [k][nbins]: lagging cells b-guard-train .. b-guard-1, leading cells b+guard+1 .. b+guard+train,
    both clipped to the row."""
    k, n = q.shape
    P = np.concatenate([np.zeros((k, 1), np.int64), np.cumsum(q, axis=1, dtype=np.int64)], axis=1)
    V = np.concatenate([np.zeros((k, 1), np.int64), np.cumsum(valid, axis=1, dtype=np.int64)], axis=1)
    b = np.arange(n)
    i0, i1 = np.maximum(b - guard - train, 0), np.maximum(b - guard, 0)
    i2, i3 = np.minimum(b + guard + 1, n), np.minimum(b + guard + 1 + train, n)
    return P[:, i1] - P[:, i0], V[:, i1] - V[:, i0], P[:, i3] - P[:, i2], V[:, i3] - V[:, i2]


def _passes(q, S, C, tq):
    lhs, rhs = q * C, S + tq * C
    assert np.abs(lhs).max(initial=0) < 2 ** 27 and np.abs(rhs).max(initial=0) < 2 ** 27      # the kernel's int32 is enough
    return (C > 0) & (lhs > rhs)


def raw_detection(q, valid, SL, CL, SR, CR, tq, mode):
    if mode == 0:
        d = _passes(q, SL + SR, CL + CR, tq)
    else:
        pl, pr = _passes(q, SL, CL, tq), _passes(q, SR, CR, tq)
        if mode == 1:
            d = ((CL > 0) | (CR > 0)) & ((CL == 0) | pl) & ((CR == 0) | pr)
        else:
            d = pl | pr
    return valid & d


def _ratio(S, C):
    with np.errstate(invalid="ignore", divide="ignore"):
        return ((S.astype(np.float32) / C.astype(np.float32)) * SCALE).astype(np.float32)


def _runs(bits):
    """(starts, ends) of the maximal runs of True in a 1-D bool array, ends exclusive."""
    edge = np.diff(np.concatenate([[0], bits.astype(np.int8), [0]]))
    return np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)


def detect(rows, train, guard, threshold_db, mode="ca", min_width=1, max_gap=0, capacity=4096, row_base=0):
    """rows float32 [k][nbins] -> dict: det0 / keep / final bool [k][nbins], count int32 [k], floor float32 [k][nbins] (the pooled
    line, NaN where there is no valid training cell), hits int64 [nbins], all (every record), events (the first `capacity`) and
    total."""
    rows = np.asarray(rows, dtype=np.float32)
    rows = rows.reshape(-1, rows.shape[-1])
    k, n = rows.shape
    mode = MODES[mode] if isinstance(mode, str) else int(mode)
    tq = threshold_q(threshold_db)
    q, valid = quantise(rows)
    SL, CL, SR, CR = window_sums(q, valid, train, guard)
    det0 = raw_detection(q, valid, SL, CL, SR, CR, tq, mode)
    floor = _ratio(SL + SR, CL + CR)
    keep, final = np.zeros_like(det0), np.zeros_like(det0)
    count = np.zeros(k, dtype=np.int32)
    recs = []
    bins = np.arange(n)
    for r in np.flatnonzero(det0.any(axis=1)):
        s, e = _runs(det0[r])
        wide = (e - s) >= min_width                              # 1. opening
        s, e = s[wide], e[wide]
        if not len(s):
            continue
        for a, b in zip(s, e):
            keep[r, a:b] = True
        first = np.concatenate([[True], (s[1:] - e[:-1]) > max_gap])    # 2. closing: the gap between two kept runs
        at = np.flatnonzero(first)
        lo, hi = s[at], e[np.concatenate([at[1:] - 1, [len(s) - 1]])] - 1
        ndet = np.add.reduceat(e - s, at)
        for a, b in zip(lo, hi):
            final[r, a:b + 1] = True
        # 3. the peak: the largest q over the keep bins, the lowest bin among equals (no keep bin lies between two emissions)
        key = np.where(keep[r], (q[r] + 65536) * 32768 + (32767 - bins), -1)
        best = np.maximum.reduceat(key, lo)
        pk = 32767 - best % 32768
        assert np.all(best >= 0) and np.all((pk >= lo) & (pk <= hi)) and np.all(keep[r, pk])
        sl, cl, sr, cr = SL[r, pk], CL[r, pk], SR[r, pk], CR[r, pk]
        if mode == 0:
            S, C = sl + sr, cl + cr
        else:
            lag = (cr == 0) | ((cl > 0) & ((sl * cr >= sr * cl) if mode == 1 else (sl * cr <= sr * cl)))
            S, C = np.where(lag, sl, sr), np.where(lag, cl, cr)
        assert np.all(C > 0)
        rec = np.zeros(len(lo), dtype=EMISSION_DTYPE)
        rec["row"], rec["bin_lo"], rec["bin_hi"], rec["peak_bin"], rec["ndet"] = r + row_base, lo, hi, pk, ndet
        rec["peak_db"], rec["floor_db"] = rows[r, pk], _ratio(S, C)
        recs.append(rec)
        count[r] = len(lo)
    every = np.concatenate(recs) if recs else np.zeros(0, dtype=EMISSION_DTYPE)
    return dict(det0=det0, keep=keep, final=final, count=count, floor=floor, hits=final.sum(axis=0).astype(np.int64),
                all=every, events=every[:capacity].copy(), total=int(len(every)))


def emissions_equal(a, b):
    """Field by field, exactly (peak_db and floor_db by their bits)."""
    if a.shape != b.shape or a.dtype != EMISSION_DTYPE or b.dtype != EMISSION_DTYPE:
        return False
    return all(np.array_equal(a[n].view(np.int32) if a[n].dtype == np.float32 else a[n],
                              b[n].view(np.int32) if b[n].dtype == np.float32 else b[n]) for n in EMISSION_DTYPE.names)


def floors_equal(a, b):
    """The floor lines: NaN in the same places, the same bits elsewhere."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.int32), b[ok].view(np.int32))


def emission_freqs(ev, freqs):
    f = np.asarray(freqs, dtype=np.float64)
    step = (f[-1] - f[0]) / (len(f) - 1)
    return (f[ev["bin_lo"]] + f[ev["bin_hi"]]) / 2, (ev["bin_hi"] - ev["bin_lo"] + 1) * step
