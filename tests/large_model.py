"""Expected results of LARGE inputs from small model runs, for tests/test_gpu_large_counts.py (the helpers themselves are proved
against the full models on the CPU, in tests/test_large_model_host.py).

The companion libraries change code path once a count crosses a threshold (a second launch, a second trip round a tile loop, a
serial stretch per thread of a one-workgroup scan), and the numpy models are far too slow at those counts.  Every result used
here is local to a row, a block or a copy, so a large input is built from a small pool and its expected result is the pool's,
gathered:

- rows (detect, mask): rows = pool[idx]; the records of row r are those of pool row idx[r] with row = base + r, the hits are
  bincount(idx) @ the hits of every pool row, row_count / row_event / floor are gathered;
- blocks (corr): the input is pool[idx] laid end to end; the records of block b are those of pool block idx[b] with block = b;
- copies (track): k copies of one list, copy j shifted by j * (rows + row_gap + 2) rows, so that nothing links across copies;
  the records of copy j are the list's with rows, first_span and labels shifted.

Nothing here is a model of its own: every value comes out of detect_model, mask_model, corr_model or track_model."""
import os
import re

import numpy as np

import corr_model as cm
import detect_model as dm
import mask_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "prgs-sdr-kspecanal_amd")


# -- the constants of the sources that the size tests mirror -------------------------------------------------------------------
def source_constant(path, name):
    """The integer a `constexpr <type> NAME = <expr>;` line of a source file gives (or one declarator of such a line:
    `constexpr int A = <expr>, NAME = <expr>;`); expr is integer literals, <<, *, / (of integers) and names defined the same way
    in the same file.  Raises when the line is not there: a constant that moved must be noticed."""
    with open(os.path.join(PKG_DIR, path)) as f:
        text = f.read()
    m = re.search(r"constexpr\s+(?:long long|int)\s+(?:[^;]*?,\s*)?%s\s*=\s*([^;,]+)[;,]" % re.escape(name), text)
    if not m:
        raise LookupError("%s defines no constexpr %s" % (path, name))
    expr = re.sub(r"(?<=[0-9])(?:ll|LL)\b", "", m.group(1))
    expr = re.sub(r"[A-Za-z_][A-Za-z_0-9]*", lambda n: str(source_constant(path, n.group(0))), expr)
    if not re.fullmatch(r"[0-9<*/\s]+", expr):
        raise ValueError("%s: %s = %s is no integer expression" % (path, name, m.group(1)))
    return int(eval(expr.replace("/", "//"), {"__builtins__": {}}))     # digits, <<, * and integer division only


def mirrored_constants():
    """dict of every constant the GPU size tests rely on, read from the source text."""
    return {
        "detect.MAX_LAUNCH_ROWS": source_constant("csrc_detect/kse_api.hip", "MAX_LAUNCH_ROWS"),
        "mask.MAX_LAUNCH_ROWS": source_constant("csrc_mask/ksm_api.hip", "MAX_LAUNCH_ROWS"),
        "detect.STAGE_BYTES": source_constant("csrc_detect/kse_api.hip", "STAGE_BYTES"),
        "mask.STAGE_BYTES": source_constant("csrc_mask/ksm_api.hip", "STAGE_BYTES"),
        "density.STAGE_BYTES": source_constant("csrc_density/ksd_api.hip", "STAGE_BYTES"),
        "resamp.GRID_MAX": source_constant("csrc_resamp/krs_api.hip", "GRID_MAX"),
        "corr.WG_PER_CU": source_constant("csrc_corr/kcr_api.hip", "WG_PER_CU"),
        "track.SCAN_THREADS": source_constant("csrc_track/ktr_kernels.hpp", "SCAN_THREADS"),
        "track.THREADS": source_constant("csrc_track/ktr_kernels.hpp", "THREADS"),
        "pulse.THREADS": source_constant("csrc_pulse/kpl_kernels.hpp", "THREADS"),
        "pulse.PER": source_constant("csrc_pulse/kpl_kernels.hpp", "PER"),
        "pulse.TILE": source_constant("csrc_pulse/kpl_kernels.hpp", "TILE"),
        # the launch plans that tests/companion_sweep.py mirrors
        "ddc.SPAN_SMALL": source_constant("csrc_ddc/kdc_api.hip", "SPAN_SMALL"),
        "ddc.SPAN_LARGE": source_constant("csrc_ddc/kdc_api.hip", "SPAN_LARGE"),
        "ddc.TILE_THREADS": source_constant("csrc_ddc/kdc_kernels.hpp", "TILE_THREADS"),
        "ddc.RED_THREADS": source_constant("csrc_ddc/kdc_kernels.hpp", "RED_THREADS"),
        "ddc.RED_WAVES": source_constant("csrc_ddc/kdc_kernels.hpp", "RED_WAVES"),
        "ddc.RED_OUT": source_constant("csrc_ddc/kdc_kernels.hpp", "RED_OUT"),
        "ddc.RED_CHUNK": source_constant("csrc_ddc/kdc_kernels.hpp", "RED_CHUNK"),
        "demod.SPAN_FOUR": source_constant("csrc_demod/kdm_api.hip", "SPAN_FOUR"),
        "demod.SPAN_TWO": source_constant("csrc_demod/kdm_api.hip", "SPAN_TWO"),
        "demod.THREADS": source_constant("csrc_demod/kdm_kernels.hpp", "THREADS"),
        "resamp.LDS_FOUR": source_constant("csrc_resamp/krs_kernels.hpp", "LDS_FOUR"),
        "resamp.THREADS": source_constant("csrc_resamp/krs_kernels.hpp", "THREADS"),
        "chan.LDS_TWO": source_constant("csrc_chan/kch_api.hip", "LDS_TWO"),
        "chan.LDS_ONE": source_constant("csrc_chan/kch_api.hip", "LDS_ONE"),
        "chan.WORK_VALUES": source_constant("csrc_chan/kch_api.hip", "WORK_VALUES"),
        "chan.MAX_W": source_constant("csrc_chan/kch_api.hip", "MAX_W"),
        "corr.THREADS": source_constant("csrc_corr/kcr_kernels.hpp", "THREADS"),
    }


EXPECTED_CONSTANTS = {
    "detect.MAX_LAUNCH_ROWS": 1 << 20, "mask.MAX_LAUNCH_ROWS": 1 << 20,
    "detect.STAGE_BYTES": 64 << 20, "mask.STAGE_BYTES": 64 << 20, "density.STAGE_BYTES": 64 << 20,
    "resamp.GRID_MAX": 1 << 20, "corr.WG_PER_CU": 16, "track.SCAN_THREADS": 1024, "track.THREADS": 256,
    "pulse.THREADS": 256, "pulse.PER": 8, "pulse.TILE": 2048,
    "ddc.SPAN_SMALL": 7680, "ddc.SPAN_LARGE": 17408, "ddc.TILE_THREADS": 256, "ddc.RED_THREADS": 512, "ddc.RED_WAVES": 8,
    "ddc.RED_OUT": 8, "ddc.RED_CHUNK": 8192, "demod.SPAN_FOUR": 9728, "demod.SPAN_TWO": 19968, "demod.THREADS": 256,
    "resamp.LDS_FOUR": 40 * 1024, "resamp.THREADS": 256, "chan.LDS_TWO": 80 * 1024, "chan.LDS_ONE": 160 * 1024,
    "chan.WORK_VALUES": 8192, "chan.MAX_W": 256, "corr.THREADS": 256,
}


# -- pools -----------------------------------------------------------------------------------------------------------------------------
def detect_pool(nrows, nbins, seed=4242, without_combs=False):
    """(pool float32 [nrows][nbins] from test_gpu_detect's own cloud: quiet rows, composite rows, all-NaN, all -inf, constant
    and every-other-bin rows; the pool rows an index may name).  without_combs leaves the every-other-bin rows (nbins / 2
    emissions each) out of the candidates: at 16384 bins a few of them alone would fill the largest emission list."""
    from test_gpu_detect import cloud
    pool = cloud(seed + nbins, nrows, nbins)
    r = np.arange(nrows)
    comb = (r % 3 == 0) & ((r // 3) % 6 == 4)                    # cloud(): kind 4
    assert nrows == 3 or np.all(pool[comb][:, ::2] == np.float32(-65.0))
    return pool, (np.flatnonzero(~comb) if without_combs else r)


def mask_pool(nrows, nbins, with_lower=True, seed=777):
    """(pool float32 [nrows][nbins] from test_gpu_mask's own cloud: every third row holds infinities, NaN, values on and one
    ulp either side of a line; upper; lower or None)."""
    from test_gpu_mask import cloud, lines_for
    up, lo = lines_for(nbins, with_lower)
    return cloud(seed + nbins, nrows, nbins, up, lo), up, lo


def corr_pool(shape, nblocks, block_len, seed):
    """(templates, pool complex64 [nblocks][block_len]): exact samples with scaled copies of the templates planted in most
    blocks, one block of zeros (windows of no energy) and one without a copy."""
    K, Q = shape
    rng = np.random.default_rng(seed)
    c = cm.exact_templates(rng, Q, K)
    pool = np.stack([cm.exact_samples(rng, block_len) for _ in range(nblocks)])
    for b in range(nblocks):
        if b % 8 == 5:
            continue
        for i in range(1 + b % 3):
            at = int(rng.integers(0, block_len - K + 1))
            pool[b, at:at + K] = (1 + (b + i) % 3) * c[(b + i) % Q]
    pool[nblocks - 2] = 0
    return c, pool


def draw(rng, candidates, n):
    """n seeded random picks among the candidate pool rows."""
    return np.asarray(candidates, dtype=np.int64)[rng.integers(0, len(candidates), n)]


# -- gathering groups of records ---------------------------------------------------------------------------------------------------
def gather_groups(records, counts, idx, limit=None):
    """records: the groups of a pool laid end to end, counts[p] records for pool item p, in pool order.  Returns (the records
    of the items idx[0], idx[1], ... laid end to end: a copy; the position in idx every one of them belongs to; the total),
    cut after the first `limit` records (the total counts them all)."""
    counts = np.asarray(counts, dtype=np.int64)
    idx = np.asarray(idx, dtype=np.int64)
    assert int(counts.sum()) == len(records)
    start = np.concatenate([[0], np.cumsum(counts)])[:-1]
    reps = counts[idx]
    total = int(reps.sum())
    if limit is not None and total > limit:                      # the items that hold the first `limit` records
        last = int(np.searchsorted(np.cumsum(reps), limit, "left")) + 1
        idx, reps = idx[:last], reps[:last]
    item = np.repeat(np.arange(len(idx), dtype=np.int64), reps)
    within = np.arange(len(item), dtype=np.int64) - np.repeat(np.cumsum(reps) - reps, reps)
    src = start[idx[item]] + within
    if limit is not None:
        src, item = src[:limit], item[:limit]
    return records[src].copy(), item, total


# -- rows: detect ----------------------------------------------------------------------------------------------------------------------
def detect_pool_model(pool, train, guard, threshold_db, mode, min_width=1, max_gap=0):
    """The model on the pool, once, with row_base 0 and room for every record."""
    want = dm.detect(pool, train, guard, threshold_db, mode, min_width, max_gap, capacity=1 << 30, row_base=0)
    assert want["total"] == len(want["all"]) == int(want["count"].sum())
    return want


def detect_expand(pool_want, idx, row_base=0, capacity=1 << 20, floor_rows=None):
    """What dm.detect gives on pool[idx] with this row_base and capacity, from its result on the pool: dict(count, hits, total,
    events, and floor: the floor lines of the rows floor_rows, or None)."""
    idx = np.asarray(idx, dtype=np.int64)
    pool_n = len(pool_want["count"])
    ev, item, total = gather_groups(pool_want["all"], pool_want["count"], idx, capacity)
    ev["row"] = row_base + item
    used = np.bincount(idx, minlength=pool_n).astype(np.int64)
    hits = used @ pool_want["final"].astype(np.int64)
    floor = None if floor_rows is None else pool_want["floor"][idx[np.asarray(floor_rows, dtype=np.int64)]]
    return dict(count=pool_want["count"][idx].astype(np.int32), hits=hits.astype(np.int64), total=total, events=ev, floor=floor)


# -- rows: mask ------------------------------------------------------------------------------------------------------------------------
def mask_pool_model(pool, upper, lower, min_bins=1):
    """The model on the pool, once, and on every pool row alone for its hits: dict(whole, row_hits int64 [P][3][nbins])."""
    whole = mm.check(pool, upper, lower, min_bins, capacity=len(pool) + 1, row_base=0)
    row_hits = np.stack([mm.check(pool[r:r + 1], upper, lower, min_bins)["hits"] for r in range(len(pool))])
    assert np.array_equal(row_hits.sum(axis=0), whole["hits"])
    return dict(whole=whole, row_hits=row_hits)


def mask_expand(pool_want, idx, row_base=0, capacity=1 << 20):
    """What mm.check gives on pool[idx] with this row_base and capacity: dict(event, hits, total, events)."""
    idx = np.asarray(idx, dtype=np.int64)
    whole = pool_want["whole"]
    event = whole["event"][idx]
    which = np.flatnonzero(event)
    keep = which[:capacity]
    ev = np.zeros(len(keep), dtype=mm.EVENT_DTYPE)
    ev["row"] = keep + row_base
    for name in ("nover", "nunder", "nnan", "peak_bin", "peak_excess", "peak_kind"):
        ev[name] = whole[name][idx[keep]]
    used = np.bincount(idx, minlength=len(whole["event"])).astype(np.int64)
    hits = np.einsum("p,pkb->kb", used, pool_want["row_hits"].astype(np.int64))
    return dict(event=event, hits=hits.astype(np.int64), total=int(len(which)), events=ev)


def rows_of(events, rows):
    """The records whose row is one of `rows`, in order."""
    return events[np.isin(events["row"], np.asarray(rows, dtype=np.int64))]


# -- blocks: corr ----------------------------------------------------------------------------------------------------------------------
def corr_pool_model(pool, templates, threshold, G, min_energy=0.0):
    """cm.exact_model and cm.records of every pool block (exact inputs): dict(rho [P][Q][lags], r, records laid end to end with
    block = 0, counts [P])."""
    rho, r, recs = [], [], []
    for block in pool:
        a, b = cm.exact_model(block, templates, min_energy)
        rho.append(a)
        r.append(b)
        recs.append(cm.records(a, b, threshold, G, block=0))
    return dict(rho=np.stack(rho), r=np.stack(r), records=np.concatenate(recs), counts=np.array([len(v) for v in recs], dtype=np.int64))


def corr_expand(pool_want, idx, capacity=1 << 20):
    """(the event list of the block form on pool[idx] laid end to end, events_total)."""
    ev, item, total = gather_groups(pool_want["records"], pool_want["counts"], idx, capacity)
    ev["block"] = item
    return ev, total


# -- copies: track ---------------------------------------------------------------------------------------------------------------------
def copy_shift(spans, row_gap):
    """Rows between two copies' first rows: the rows the list spans, and row_gap + 2 more, so the next copy begins beyond reach."""
    return int(spans["row"][-1]) - int(spans["row"][0]) + 1 + row_gap + 2


def track_copies(spans, k, row_gap):
    """(k copies of the list laid end to end, a row_end more than row_gap + 1 beyond the last row)."""
    shift = copy_shift(spans, row_gap)
    out = np.concatenate([spans] * k)
    out["row"] += np.repeat(np.arange(k, dtype=np.int64) * shift, len(spans))
    return out, int(out["row"][-1]) + 1 + row_gap + 2


def track_expand(want, spans, k, row_gap, capacity=1 << 20):
    """What tm.link gives on track_copies(spans, k, row_gap), from `want` = its result on `spans` alone (with every record
    stored and a row_end that leaves no track open): (records, tracks_total, components_total, labels, 0)."""
    rec, total, comps, labels, bad = want
    assert bad == 0 and len(rec) == total and not rec["flags"].any()
    shift, n0 = copy_shift(spans, row_gap), len(spans)
    out = np.concatenate([rec] * k)
    j = np.repeat(np.arange(k, dtype=np.int64), len(rec))
    for name in ("row_first", "row_last", "peak_row"):
        out[name] += j * shift
    out["first_span"] += (j * n0).astype(np.int32)
    lab = np.concatenate([labels] * k).astype(np.int64)
    lab = np.where(lab >= 0, lab + np.repeat(np.arange(k, dtype=np.int64) * total, n0), -1).astype(np.int32)
    return out[:capacity].copy(), total * k, comps * k, lab, 0
