"""The contract of survey.stitch_emissions once more, by brute force and in plain Python: every band record is judged on its own
(the edge rule by trying every other band), the survivors of a pass are painted into an array over the stitched range and the
runs of painted elements are read back -- no sorting, no sweep.  It is the yardstick of the host and of the GPU tests; the
function under test is never compared with itself."""
import numpy as np

EMISSION_DTYPE = np.dtype([("row", "<i8"), ("bin_lo", "<i4"), ("bin_hi", "<i4"), ("peak_bin", "<i4"), ("ndet", "<i4"),
                           ("peak_db", "<f4"), ("floor_db", "<f4")])
COUNTERS = ("dc_dropped", "edge_dropped", "clipped")


def records_of(rows):
    """EMISSION_DTYPE records from tuples (row, bin_lo, bin_hi[, peak_bin[, peak_db[, floor_db[, ndet]]]]): the peak defaults to
    bin_lo at -50 dB over a floor of -90 dB, ndet to the width."""
    out = np.zeros(len(rows), dtype=EMISSION_DTYPE)
    for i, r in enumerate(rows):
        out[i]["row"], out[i]["bin_lo"], out[i]["bin_hi"] = r[0], r[1], r[2]
        out[i]["peak_bin"] = r[3] if len(r) > 3 else r[1]
        out[i]["peak_db"] = r[4] if len(r) > 4 else -50.0
        out[i]["floor_db"] = r[5] if len(r) > 5 else -90.0
        out[i]["ndet"] = r[6] if len(r) > 6 else r[2] - r[1] + 1
    return out


def survives(r, steps, hop, nbins, total, edge, dc, counters):
    """None when a rule drops the band record r (and counts it), else (pass, band, lo, hi, peak) in stitched elements."""
    p, s = divmod(int(r["row"]), steps)
    lo, hi, pk = int(r["bin_lo"]), int(r["bin_hi"]), int(r["peak_bin"])
    if dc > 0 and nbins // 2 - dc <= lo and hi <= nbins // 2 + dc:
        counters["dc_dropped"] += 1
        return None
    e = s * hop + pk
    if edge > 0 and (pk < edge or pk >= nbins - edge):
        if any(edge <= e - t * hop < nbins - edge for t in range(steps) if t != s):
            counters["edge_dropped"] += 1
            return None
    if e >= total:
        counters["clipped"] += 1
        return None
    return p, s, s * hop + lo, min(s * hop + hi, total - 1), e


def stitch(records, steps, hop, nbins, total, edge=0, dc=0):
    """(stitched, members, counters) as survey.stitch_emissions states them."""
    counters = dict.fromkeys(COUNTERS, 0)
    by_pass = {}
    for i, r in enumerate(records):
        got = survives(r, steps, hop, nbins, total, edge, dc, counters)
        if got is not None:
            by_pass.setdefault(got[0], []).append((i,) + got[1:])
    out, members = [], []
    for p in sorted(by_pass):
        paint = np.zeros(total + 2, dtype=np.int8)          # one spare element on either side: every run ends inside
        for _, _, lo, hi, _ in by_pass[p]:
            paint[lo + 1:hi + 2] = 1
        step = np.diff(paint)
        for a, b in zip(np.flatnonzero(step == 1), np.flatnonzero(step == -1) - 1):
            inside = [m for m in by_pass[p] if a <= m[2] <= b]
            assert all(m[3] <= b for m in inside)
            i, s, _, _, e = max(inside, key=lambda m: (float(records[m[0]]["peak_db"]), -m[4], -m[1]))
            rec = np.zeros((), dtype=EMISSION_DTYPE)
            rec["row"], rec["bin_lo"], rec["bin_hi"], rec["peak_bin"] = p, a, b, e
            rec["ndet"] = min(sum(int(records[m[0]]["ndet"]) for m in inside), b - a + 1)
            rec["peak_db"], rec["floor_db"] = records[i]["peak_db"], records[i]["floor_db"]
            out.append(rec)
            members.append(len(inside))
    stitched = np.array(out, dtype=EMISSION_DTYPE) if out else np.zeros(0, dtype=EMISSION_DTYPE)
    return stitched, np.array(members, dtype=np.int32), counters


def occupancy(stitched, npasses, total, cells):
    """int64 [cells]: the passes in which a stitched record touched the cell of total / cells elements."""
    g = total // cells
    occ = np.zeros(cells, dtype=np.int64)
    for p in range(npasses):
        hit = np.zeros(cells, dtype=bool)
        for r in stitched[stitched["row"] == p]:
            hit[int(r["bin_lo"]) // g:int(r["bin_hi"]) // g + 1] = True
        occ += hit
    return occ


def same_records(a, b):
    """Equality of two record arrays by their bytes."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def random_band_records(steps, hop, nbins, npasses, seed, p=0.25, empty_pass=None):
    """Seeded band records of npasses passes: a random scene over the elements all bands cover, of which every band sees its own
    window with some bins flipped, so that the sightings of overlapping bands overlap, nest, abut and differ; peak_db comes from
    a handful of values, so that two bands often report equal peaks.  The pass `empty_pass` has no record."""
    rng = np.random.default_rng(seed)
    rows = []
    for q in range(npasses):
        if q == empty_pass:
            continue
        scene = rng.random((steps - 1) * hop + nbins) < p
        for s in range(steps):
            seen = scene[s * hop:s * hop + nbins] ^ (rng.random(nbins) < 0.08)
            edge = np.flatnonzero(np.diff(np.concatenate(([0], seen.astype(np.int8), [0]))))
            for lo, hi in zip(edge[0::2], edge[1::2] - 1):
                rows.append((q * steps + s, int(lo), int(hi), int(rng.integers(lo, hi + 1)), float(rng.integers(-4, 0)) * 10.0,
                             -90.0 + float(rng.integers(0, 3)), int(rng.integers(1, hi - lo + 2))))
    return records_of(rows)
