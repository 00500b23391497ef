"""The contract of include/ksa_track.h in numpy and plain Python: a sequential union-find over the adjacency rule and the
reductions, written for clarity and not for speed.  It is the only yardstick of the GPU tests: the GPU is never compared with
itself."""
import numpy as np

FLAG_OPEN_END = 1

SPAN_DTYPE = np.dtype([("row", "<i8"), ("bin_lo", "<i4"), ("bin_hi", "<i4"), ("peak_bin", "<i4"), ("ndet", "<i4"),
                       ("peak_db", "<f4"), ("floor_db", "<f4")])
TRACK_DTYPE = np.dtype([("row_first", "<i8"), ("row_last", "<i8"), ("peak_row", "<i8"), ("cells", "<i8"), ("sum_mid2", "<i8"),
                        ("bin_lo", "<i4"), ("bin_hi", "<i4"), ("nspans", "<i4"), ("peak_bin", "<i4"), ("mid2_first", "<i4"),
                        ("mid2_last", "<i4"), ("first_span", "<i4"), ("flags", "<i4"), ("peak_db", "<f4"), ("floor_db", "<f4")])


def spans_of(rows):
    """SPAN_DTYPE records from tuples (row, bin_lo, bin_hi[, peak_db[, floor_db[, peak_bin]]]); peak_db defaults to 0."""
    out = np.zeros(len(rows), dtype=SPAN_DTYPE)
    for i, r in enumerate(rows):
        out[i]["row"], out[i]["bin_lo"], out[i]["bin_hi"] = r[0], r[1], r[2]
        out[i]["peak_db"] = r[3] if len(r) > 3 else 0.0
        out[i]["floor_db"] = r[4] if len(r) > 4 else -100.0
        out[i]["peak_bin"] = r[5] if len(r) > 5 else r[1]
        out[i]["ndet"] = r[2] - r[1] + 1
    return out


def key(peak_db):
    """The order of float32 bit patterns: ~u when the sign bit is set, u | 0x80000000 otherwise."""
    u = int(np.asarray(peak_db, dtype=np.float32).view(np.uint32))
    return (~u) & 0xFFFFFFFF if u & 0x80000000 else u | 0x80000000


def bad_indices(spans, nbins, row_end):
    """Every index that breaks a validity rule, ascending."""
    row, lo, hi = (spans[k].astype(np.int64) for k in ("row", "bin_lo", "bin_hi"))
    bad = (lo < 0) | (lo > hi) | (hi >= nbins) | (row < 0) | (row >= row_end)
    if len(spans) > 1:
        after = (row[1:] > row[:-1]) | ((row[1:] == row[:-1]) & (lo[1:] > lo[:-1]) & (lo[1:] > hi[:-1]))
        bad[1:] |= ~after
    return np.flatnonzero(bad)


def adjacent(a, b, row_gap, bin_slop):
    """Spans a (the earlier) and b by the rule, in Python integers."""
    dr = int(b["row"]) - int(a["row"])
    return (1 <= dr <= 1 + row_gap and int(a["bin_lo"]) <= int(b["bin_hi"]) + bin_slop
            and int(b["bin_lo"]) <= int(a["bin_hi"]) + bin_slop)


def components(spans, row_gap, bin_slop):
    """root[i] = the lowest index of the component of span i: a sequential union-find over every adjacent pair."""
    n = len(spans)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    row = spans["row"].astype(np.int64)
    lo, hi = spans["bin_lo"].astype(np.int64), spans["bin_hi"].astype(np.int64)
    for i in range(n):
        # the later rows within reach are one slice of the sorted list; the rule is applied to every span of it
        j0, j1 = np.searchsorted(row, row[i], "right"), np.searchsorted(row, row[i] + 1 + row_gap, "right")
        for j in j0 + np.flatnonzero((lo[i] <= hi[j0:j1] + bin_slop) & (lo[j0:j1] <= hi[i] + bin_slop)):
            a, b = find(i), find(int(j))
            if a != b:
                parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)], dtype=np.int64)


def link(spans, nbins, row_end, row_gap=0, bin_slop=0, min_rows=1, min_spans=1, capacity=4096):
    """(records of the first `capacity` tracks, tracks_total, components_total, labels int32 [n], bad_spans)."""
    spans = np.asarray(spans)
    n = len(spans)
    bad = bad_indices(spans, nbins, row_end)
    if len(bad):
        return np.zeros(0, dtype=TRACK_DTYPE), 0, 0, np.full(n, -1, dtype=np.int32), len(bad)
    root = components(spans, row_gap, bin_slop)
    members = {}
    for i in range(n):
        members.setdefault(int(root[i]), []).append(i)
    records, labels, rank = [], np.full(n, -1, dtype=np.int32), 0
    for first in sorted(members):
        idx = members[first]
        m = spans[idx]
        row_first, row_last = int(m["row"].min()), int(m["row"].max())
        if row_last - row_first + 1 < min_rows or len(idx) < min_spans:
            continue
        peak = max(idx, key=lambda i: (key(spans[i]["peak_db"]), -i))
        rec = np.zeros((), dtype=TRACK_DTYPE)
        rec["row_first"], rec["row_last"], rec["peak_row"] = row_first, row_last, spans[peak]["row"]
        rec["cells"] = int((m["bin_hi"].astype(np.int64) - m["bin_lo"] + 1).sum())
        rec["sum_mid2"] = int((m["bin_hi"].astype(np.int64) + m["bin_lo"]).sum())
        rec["bin_lo"], rec["bin_hi"], rec["nspans"] = m["bin_lo"].min(), m["bin_hi"].max(), len(idx)
        rec["peak_bin"] = spans[peak]["peak_bin"]
        rec["mid2_first"] = int(spans[idx[0]]["bin_lo"]) + int(spans[idx[0]]["bin_hi"])
        rec["mid2_last"] = int(spans[idx[-1]]["bin_lo"]) + int(spans[idx[-1]]["bin_hi"])
        rec["first_span"] = first
        rec["flags"] = FLAG_OPEN_END if row_last + row_gap + 1 >= row_end else 0
        rec["peak_db"], rec["floor_db"] = spans[peak]["peak_db"], spans[peak]["floor_db"]      # float32 to float32: the bits
        labels[idx] = rank
        if rank < capacity:
            records.append(rec)
        rank += 1
    out = np.array(records, dtype=TRACK_DTYPE) if records else np.zeros(0, dtype=TRACK_DTYPE)
    return out, rank, len(members), labels, 0


def same_records(a, b):
    """Equality of two record arrays by their bytes: NaN peaks and the sign of zero count."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def random_occupancy(nrows, nbins=64, p=0.18, seed=1, row0=0):
    """Spans from a seeded random occupancy [nrows][nbins]: every maximal run of occupied bins of a row is one span; peak_db a
    seeded float32 rounded to 1/4 dB so that ties occur."""
    rng = np.random.default_rng(seed)
    occ = rng.random((nrows, nbins)) < p
    rows = []
    for r in range(nrows):
        edge = np.flatnonzero(np.diff(np.concatenate(([0], occ[r].astype(np.int8), [0]))))
        for lo, hi in zip(edge[0::2], edge[1::2] - 1):
            rows.append((row0 + r, int(lo), int(hi)))
    out = spans_of(rows)
    out["peak_db"] = (np.round(rng.normal(-60, 6, len(out)) * 4) / 4).astype(np.float32)
    out["floor_db"] = (out["peak_db"] - np.float32(12.5)).astype(np.float32)
    out["peak_bin"] = out["bin_lo"] + (out["bin_hi"] - out["bin_lo"]) // 2
    return out


def times_freqs(tracks, freqs, row_period_s):
    """The derived arrays of track.track_times_freqs, written out once more."""
    f = np.asarray(freqs, dtype=np.float64)
    step = (f[-1] - f[0]) / (len(f) - 1) if len(f) > 1 else 0.0
    out = {k: np.zeros(len(tracks), dtype=np.float64) for k in ("t_start_s", "duration_s", "center_hz", "width_hz", "drift_hz_per_s")}
    for i, t in enumerate(tracks):
        rows = int(t["row_last"]) - int(t["row_first"])
        out["t_start_s"][i] = float(int(t["row_first"])) * row_period_s
        out["duration_s"][i] = float(rows + 1) * row_period_s
        out["center_hz"][i] = (f[t["bin_lo"]] + f[t["bin_hi"]]) / 2
        out["width_hz"][i] = float(int(t["bin_hi"]) - int(t["bin_lo"]) + 1) * step
        if rows > 0 and row_period_s > 0:
            out["drift_hz_per_s"][i] = (float(t["mid2_last"]) - float(t["mid2_first"])) / 2 * step / (float(rows) * row_period_s)
    return out
