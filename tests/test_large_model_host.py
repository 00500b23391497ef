"""tests/large_model.py against the full models, on the CPU, at sizes where the full models are still affordable: the expected
results of tests/test_gpu_large_counts.py are gathered from small pools, and the gathering must be exactly what the model gives
on the large input.  Every helper also gets one corrupted expansion, which the equality function its GPU test uses must notice.
The constants of the sources that the size tests mirror are pinned here from the source text."""
import numpy as np
import pytest

import corr_model as cm
import detect_model as dm
import large_model as lm
import mask_model as mm
import track_model as tm

THRESHOLD = 10.0


# ------------------------------------------------------------------------------------------ the mirrored constants
def test_the_source_constants_are_the_ones_the_size_tests_mirror():
    got = lm.mirrored_constants()
    assert got == lm.EXPECTED_CONSTANTS, {k: (got[k], lm.EXPECTED_CONSTANTS[k]) for k in got if got[k] != lm.EXPECTED_CONSTANTS.get(k)}
    assert got["pulse.TILE"] == got["pulse.THREADS"] * got["pulse.PER"]
    with pytest.raises(LookupError):
        lm.source_constant("csrc_corr/kcr_api.hip", "NO_SUCH_CONSTANT")


def test_gather_groups_on_a_hand_made_list():
    rec = np.array([10, 11, 20, 40, 41, 42])                     # pool item 0: two records, 1: one, 2: none, 3: three
    counts = [2, 1, 0, 3]
    out, item, total = lm.gather_groups(rec, counts, [3, 2, 0, 0, 1])
    assert list(out) == [40, 41, 42, 10, 11, 10, 11, 20] and list(item) == [0, 0, 0, 2, 2, 3, 3, 4] and total == 8
    for limit in range(9):
        cut, item2, total = lm.gather_groups(rec, counts, [3, 2, 0, 0, 1], limit)
        assert list(cut) == list(out[:limit]) and list(item2) == list(item[:limit]) and total == 8
    out, item, total = lm.gather_groups(rec, counts, [2, 2])
    assert len(out) == 0 and len(item) == 0 and total == 0


# ------------------------------------------------------------------------------------------ rows: detect
@pytest.mark.parametrize("mode,min_width,max_gap", [("ca", 1, 0), ("go", 1, 2), ("so", 3, 0)])
def test_detect_rows_gathered_from_a_pool_equal_the_model(mode, min_width, max_gap):
    nbins, train, guard, base = 16, 4, 1, 2 ** 33
    pool, cand = lm.detect_pool(64, nbins)
    idx = lm.draw(np.random.default_rng(1), cand, 3000)
    assert len(np.unique(idx)) == 64
    want = lm.detect_pool_model(pool, train, guard, THRESHOLD, mode, min_width, max_gap)
    full = dm.detect(pool[idx], train, guard, THRESHOLD, mode, min_width, max_gap, capacity=1 << 20, row_base=base)
    assert full["total"] > 200 and (full["count"] == 0).sum() > 500, "the case needs quiet and busy rows"
    floor_rows = np.arange(0, 3000, 7)
    got = lm.detect_expand(want, idx, base, 1 << 20, floor_rows)
    assert dm.emissions_equal(got["events"], full["events"]) and got["total"] == full["total"]
    assert np.array_equal(got["count"], full["count"]) and got["count"].dtype == full["count"].dtype
    assert np.array_equal(got["hits"], full["hits"]) and got["hits"].dtype == full["hits"].dtype
    assert dm.floors_equal(got["floor"], full["floor"][floor_rows])
    assert np.isnan(got["floor"]).any(), "rows without a valid training cell are among the compared ones"
    # a capacity below the total keeps the first records
    cut = lm.detect_expand(want, idx, base, 777)
    assert cut["total"] == full["total"] and dm.emissions_equal(cut["events"], full["events"][:777])
    # one row index off is noticed
    off = idx.copy()
    k = int(np.flatnonzero(full["count"] > 0)[5])
    off[k] = cand[(int(np.flatnonzero(cand == idx[k])[0]) + 1) % len(cand)]
    bad = lm.detect_expand(want, off, base)
    assert not dm.emissions_equal(bad["events"], full["events"])
    shifted = got["events"].copy()
    shifted["row"][10] += 1
    assert not dm.emissions_equal(shifted, full["events"])


# ------------------------------------------------------------------------------------------ rows: mask
@pytest.mark.parametrize("with_lower,min_bins", [(True, 1), (False, 3)])
def test_mask_rows_gathered_from_a_pool_equal_the_model(with_lower, min_bins):
    nbins, base = 16, 2 ** 33
    pool, up, lo = lm.mask_pool(64, nbins, with_lower)
    idx = lm.draw(np.random.default_rng(2), np.arange(64), 3000)
    want = lm.mask_pool_model(pool, up, lo, min_bins)
    full = mm.check(pool[idx], up, lo, min_bins, capacity=1 << 20, row_base=base)
    assert 200 < full["total"] < 2500, "the case needs event rows and quiet rows"
    got = lm.mask_expand(want, idx, base)
    assert mm.events_equal(got["events"], full["events"]) and got["total"] == full["total"]
    assert np.array_equal(got["hits"], full["hits"]) and got["hits"].dtype == full["hits"].dtype
    assert np.array_equal(got["event"], full["event"])
    cut = lm.mask_expand(want, idx, base, 99)
    assert cut["total"] == full["total"] and mm.events_equal(cut["events"], full["events"][:99])
    assert mm.events_equal(lm.rows_of(got["events"], base + np.arange(100, 140)),
                           full["events"][(full["events"]["row"] >= base + 100) & (full["events"]["row"] < base + 140)])
    # one row index off is noticed
    off = idx.copy()
    k = int(np.flatnonzero(full["event"])[5])
    off[k] = (idx[k] + 1) % 64
    bad = lm.mask_expand(want, off, base)
    assert not (mm.events_equal(bad["events"], full["events"]) and np.array_equal(bad["hits"], full["hits"]))
    shifted = got["events"].copy()
    shifted["row"][10] += 1
    assert not mm.events_equal(shifted, full["events"])


# ------------------------------------------------------------------------------------------ blocks: corr
def events_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and all(np.array_equal(a[k], b[k]) for k in a.dtype.names)


@pytest.mark.parametrize("shape", [(7, 3), (64, 1)], ids=str)
def test_corr_blocks_gathered_from_a_pool_equal_the_model(shape):
    K, Q = shape
    G, thr, block_len = 5, 0.5, 300 + K - 1
    c, pool = lm.corr_pool(shape, 8, block_len, 11)
    idx = lm.draw(np.random.default_rng(3), np.arange(8), 40)
    want = lm.corr_pool_model(pool, c, thr, G)
    # the full model: every block of the input laid end to end, modelled on its own
    x = pool[idx].reshape(-1)
    rho = np.stack([cm.exact_model(x[b * block_len:(b + 1) * block_len], c)[0] for b in range(40)])
    r = np.stack([cm.exact_model(x[b * block_len:(b + 1) * block_len], c)[1] for b in range(40)])
    full = cm.block_records(rho, r, thr, G)
    got, total = lm.corr_expand(want, idx)
    assert total == len(full) >= 40 and events_equal(got, full)
    assert (want["counts"] == 0).any() and (want["counts"] > 1).any(), "the block of zeros has no event"
    assert np.array_equal(want["rho"][idx], rho) and np.array_equal(want["r"][idx], r)
    cut, total = lm.corr_expand(want, idx, 17)
    assert total == len(full) and events_equal(cut, full[:17])
    # one block index off is noticed
    off = idx.copy()
    off[7] = (off[7] + 1) % 8
    assert not events_equal(lm.corr_expand(want, off)[0], full)
    shifted = got.copy()
    shifted["block"][3] += 1
    assert not events_equal(shifted, full)


# ------------------------------------------------------------------------------------------ copies: track
@pytest.mark.parametrize("kw", [dict(), dict(min_rows=3)], ids=str)
def test_track_copies_equal_the_model(kw):
    nbins, row_gap, slop, k = 64, 1, 1, 3
    s = tm.random_occupancy(300, nbins, 0.18, seed=20260)[:2000]
    assert len(s) == 2000
    spans, row_end = lm.track_copies(s, k, row_gap)
    assert len(spans) == 6000 and row_end > int(spans["row"][-1]) + row_gap + 1
    one_end = int(s["row"][-1]) + 1 + row_gap + 2
    want = tm.link(s, nbins, one_end, row_gap, slop, capacity=1 << 20, **kw)
    full = tm.link(spans, nbins, row_end, row_gap, slop, capacity=1 << 20, **kw)
    assert full[4] == 0 and full[1] > 30 and full[0]["nspans"].max() >= 5
    if kw:
        assert 0 < full[1] < full[2] and (full[3] == -1).any()
    got = lm.track_expand(want, s, k, row_gap)
    assert tm.same_records(got[0], full[0]) and got[1:3] == full[1:3] and np.array_equal(got[3], full[3])
    assert got[3].dtype == full[3].dtype
    half = full[1] // 2
    cut = lm.track_expand(want, s, k, row_gap, capacity=half)
    capped = tm.link(spans, nbins, row_end, row_gap, slop, capacity=half, **kw)
    assert tm.same_records(cut[0], capped[0]) and np.array_equal(cut[3], capped[3]) and cut[1] == capped[1]
    # a gap one row shorter would link copies: the shift is the smallest that is safe for every list
    assert lm.copy_shift(s, row_gap) == int(s["row"][-1]) - int(s["row"][0]) + 1 + 3
    # one label offset off, and one row off, are noticed
    lab = got[3].copy()
    at = int(np.flatnonzero(lab >= 0)[-1])
    lab[at] += 1
    assert not np.array_equal(lab, full[3])
    rec = got[0].copy()
    rec["first_span"][len(rec) // 2] += 1
    assert not tm.same_records(rec, full[0])
    rec = got[0].copy()
    rec["row_last"][-1] += 1
    assert not tm.same_records(rec, full[0])
