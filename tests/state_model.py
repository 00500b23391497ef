"""numpy models of the state, plot and stitch half of libksa.so -- TEST INFRASTRUCTURE, NOT PRODUCT.

Written from the text of include/ksa.h and the K: lines it cites (oracle/ksa_oracle.py restates those), not from the kernels:
every model works on whole curves with slices, sorts and numpy reductions, the way the reference does, where the kernels work
one element or one cell per thread.  Float32 steps that the header pins bit for bit ((a + x) * 0.5, a rank-order sum, a cell
maximum) are taken in float32 here too; averages are taken in float64 (math.fsum, or the reference's own recursion), and the
GPU tests derive the float32 rounding they allow on top.

State layout everywhere: float32[4][n] = cur, max, min, avg (ksa_state_dev / ksa_scan_state_dev)."""
import math

import numpy as np

HM_ROWS = 128
F32 = np.float32


def _quiet():
    return np.errstate(invalid="ignore", over="ignore", divide="ignore")


# ------------------------------------------------------------------------------------------------ levels / highs / view
def _cell_avg(v, g):
    """float32(exact sum of the float32 values / g); NaN if one value is NaN or both infinities are there."""
    if np.isnan(v).any() or (np.isposinf(v).any() and np.isneginf(v).any()):
        return F32(np.nan)
    if np.isinf(v).any():
        return F32(np.inf) if np.isposinf(v).any() else F32(-np.inf)
    return F32(math.fsum(float(x) for x in v) / g)


def levels(state, adj, cells, mode):
    """ksa_read_levels: every curve of `state` ([k][n] float32) minus adj (float32, or None), cut into `cells` groups of
    g = n/cells and reduced with pltCompress `mode` (K:205-221): float32[k][cells].  MAX / MIN are numpy's (a NaN in the cell
    gives NaN); AVG is the exactly rounded mean of the float32 differences."""
    state = np.asarray(state, dtype=F32)
    k, n = state.shape
    assert n % cells == 0
    g = n // cells
    with _quiet():
        v = state if adj is None else (state - np.asarray(adj, dtype=F32)[None, :]).astype(F32)
        t = v.reshape(k, cells, g)
        mode = mode.upper()
        if mode == "MAX":
            return np.max(t, axis=2)
        if mode == "MIN":
            return np.min(t, axis=2)
        assert mode == "AVG"
        return np.array([[_cell_avg(t[c, j], g) for j in range(cells)] for c in range(k)], dtype=F32)


def highs(curve, min_sep, count):
    """ksa_read_highs on a decimated curve: (cells int list in marking order, their levels, found).  Stable ascending argsort
    read backwards (K:251-258): NaN is last in the sort and so first in the walk, equal levels -- +0.0 and -0.0 are equal --
    come higher index first, and the element at sorted position 0 is never visited.  A cell is marked unless an already
    marked one is closer than min_sep: abs(c - m) >= min_sep in float64 on integer cells (K:261-262)."""
    curve = np.asarray(curve)
    order = np.argsort(curve, kind="stable")
    marks = []
    for j in range(1, len(curve)):
        if len(marks) >= count:
            break
        c = int(order[-j])
        if all(abs(float(c - m)) >= float(min_sep) for m in marks):
            marks.append(c)
    return marks, [curve[c] for c in marks], len(marks)


def ring_rows(ring, hm_index, nrows):
    """The newest `nrows` rows of a waterfall ring whose position AFTER the newest row is hm_index, oldest first
    (ksa_read_view; K:480-484)."""
    ring = np.asarray(ring)
    return ring[[(hm_index - nrows + r) % HM_ROWS for r in range(nrows)]].reshape(nrows, ring.shape[1])


def view(state, adj, ring, hm_index, cells, mode, curve, min_sep, count, nrows):
    """ksa_read_view = ksa_read_levels + ksa_read_highs of `curve` (0..3; count 0 skips) + the newest rows + hm_index."""
    lv = levels(state, adj, cells, mode)
    marks, lvl, found = highs(lv[curve], min_sep, count) if count > 0 else ([], [], 0)
    return lv, marks, lvl, found, ring_rows(ring, hm_index, nrows), hm_index


# ------------------------------------------------------------------------------------------------ zeroSpanPlay rows
def db_rows(mag, gain, adj, width):
    """ksa_frame_spectrum (K:469, K:478-480) in float64: (10 log10(mag) - gain, the waterfall row of `width` cell maxima of
    that minus adj; NaN wins a cell).  width 0: no row."""
    mag = np.asarray(mag, dtype=np.float64)
    with _quiet():
        db = 10.0 * np.log10(mag) - float(gain)
        if not width:
            return db, None
        v = db if adj is None else db - np.asarray(adj, dtype=np.float64)
        return db, np.max(v.reshape(width, len(mag) // width), axis=1)


# ------------------------------------------------------------------------------------------------ accumulate
def accumulate(rows, first_index, total, prev, has, flags):
    """K:470-476 over the batch rows ([k][n] float32 dB rows) = frames [first_index, first_index + k) of a logical run of
    `total` frames, on top of prev ([4][n]; None on a fresh engine) whose curves max, min, avg already hold frames where
    has = (has_max, has_min, has_avg) says so; flags = (b_max, b_min, b_avg).  Returns (state, has):
      cur   the run's last frame (the batch must own it),
      max / min  numpy's maximum / minimum (NaN wins), seeded by copy the first time their flag is on,
      avg   orc.data_cumu's recursion a = (a + x) / 2 in float64 over the float32 rows, seeded by copy of frame 0 of the
            run (K:133-134); a frame of the run that is not in the batch adds nothing, i.e. a = a / 2 (that is what makes
            the sums of several shards add up to the run, ksa.h "closed form")
    as float64 arrays (cur, max, min hold float32 values)."""
    rows = np.asarray(rows, dtype=F32)
    k, n = rows.shape
    assert 0 <= first_index and first_index + k == total, "the batch must own the run's last frame"
    has_max, has_min, has_avg = (bool(h) for h in has)
    b_max, b_min, b_avg = (bool(b) for b in flags)
    out = np.zeros((4, n)) if prev is None else np.array(prev, dtype=np.float64)
    r64 = rows.astype(np.float64)
    with _quiet():
        out[0] = r64[-1]
        if b_max:
            m = np.max(r64, axis=0)
            out[1] = np.max([out[1], m], axis=0) if has_max else m
        if b_min:
            m = np.min(r64, axis=0)
            out[2] = np.min([out[2], m], axis=0) if has_min else m
        if b_avg:
            a = out[3].copy() if has_avg else None
            for kg in range(total):
                x = r64[kg - first_index] if kg >= first_index else None
                if a is None:
                    a = x.copy() if x is not None else np.zeros(n)       # (kg == 0 here)
                elif x is None:
                    a = a / 2
                else:
                    a = (a + x) / 2
            out[3] = a
    return out, (has_max or b_max, has_min or b_min, has_avg or b_avg)


def nan_max(a, b):
    """np.max of a pair, element by element: a NaN on either side wins."""
    with _quiet():
        return np.max([a, b], axis=0)


def merge_gathered(blocks, world, fpr, idx0, width, ring):
    """ksa_merge_gathered_dev: blocks = float32[world][4n + 128*width] exchange blocks in rank order ([max | cur | -min | sum]
    then the rank's ring).  Returns (partial float32[4][n], ring float32[128][width]): rows 0-2 by NaN-propagating max, the sum
    added in rank order IN FLOAT32 (exact: nothing but adds), and ring row s taken from the rank that holds the newest frame f
    of the run with (idx0 + f) % 128 == s (rank r holds frames [r*fpr, (r+1)*fpr)); a row no frame maps to keeps `ring`'s."""
    blocks = np.asarray(blocks, dtype=F32)
    n = (blocks.shape[1] - HM_ROWS * width) // 4
    part = blocks[0, :4 * n].reshape(4, n).copy()
    with _quiet():
        for r in range(1, world):
            b = blocks[r, :4 * n].reshape(4, n)
            part[:3] = nan_max(part[:3], b[:3])
            part[3] = (part[3] + b[3]).astype(F32)
    out = np.array(ring, dtype=F32).reshape(HM_ROWS, width).copy()
    total = world * fpr
    newest = {}
    for f in range(total):
        newest[(idx0 + f) % HM_ROWS] = f
    for s, f in newest.items():
        out[s] = blocks[f // fpr, 4 * n:].reshape(HM_ROWS, width)[s]
    return part, out


def commit_fresh(part):
    """The state a fresh engine holds after committing `part` ([max | cur | -min | sum]): cur, max, min, avg."""
    return np.array([part[1], part[0], -part[2], part[3]], dtype=F32)


# ------------------------------------------------------------------------------------------------ scan stitch
def stitch(bands, n, hop, total, state, first_pass, base_is_raw, flags=(True, True)):
    """ksa_scan_stitch_passes_dev: bands = float32[npasses][nsteps][n] dB spectra, state = float32[4][total].  Runs K:622-668
    pass after pass, band after band, on slices and IN FLOAT32: the first band to reach an element copies (RAW, K:643-644),
    every later one halves in, (c + x) * float32(0.5) (K:645-650; one add and one exact multiply); then Max / Min / Avg take
    the stitched Fft.Cur over the elements this band finishes ([i*hop, (i+1)*hop); the pass's last band: up to its end), or
    with base_is_raw every band's own spectrum over all its elements (K:651-668).  The first pass of a run seeds Avg by
    copy (K:615-618).  Elements no band covers keep their value.
    Returns (state float32[4][total], avg_rows float32[npasses][total] = Fft.Avg after each pass)."""
    bands = np.asarray(bands, dtype=F32)
    npasses, nsteps, _ = bands.shape
    cur, mx, mn, av = (np.array(s, dtype=F32) for s in np.asarray(state, dtype=F32).reshape(4, total))
    b_max, b_min = flags
    half = F32(0.5)
    avg_rows = np.empty((npasses, total), dtype=F32)
    with _quiet():
        for p in range(npasses):
            seed = first_pass and p == 0
            old_end = 0
            for i in range(nsteps):
                pr = bands[p, i]
                i_start = i * hop
                if i_start >= total:
                    break
                i_end = min(i_start + n, total)
                old_end = min(max(old_end, i_start), total)        # (hop <= n: old_end >= i_start already)
                cur[old_end:i_end] = pr[old_end - i_start:i_end - i_start]
                if old_end > i_start:
                    cur[i_start:old_end] = (cur[i_start:old_end] + pr[:old_end - i_start]) * half
                old_end = i_end
                if base_is_raw:
                    d0, d1, src = i_start, i_end, pr[:i_end - i_start]
                else:
                    d1 = i_end if i == nsteps - 1 else min((i + 1) * hop, total)
                    d0, src = i_start, cur[i_start:d1]
                if b_max:
                    mx[d0:d1] = np.max([mx[d0:d1], src], axis=0)
                if b_min:
                    mn[d0:d1] = np.min([mn[d0:d1], src], axis=0)
                av[d0:d1] = src if seed else (av[d0:d1] + src) * half
            avg_rows[p] = av
    return np.array([cur, mx, mn, av], dtype=F32), avg_rows


def scan_rows(avg_rows, adj, width, row0, ring=None, e_lo=0, e_hi=None):
    """K:696-697 for a batch: row p of avg_rows ([rows][total] float32) minus adj (float32), cell maxima over g = total/width
    elements with NaN winning.  ring given: the rows stored at (row0 + p) % 128 of a copy of it, which is returned;
    ring None: the rows themselves.  e_lo / e_hi: the PARTIAL rows of a shard that owns elements [e_lo, e_hi) only --
    -inf where it owns nothing of a cell (ksa_scan_stitch_range_dev)."""
    avg_rows = np.asarray(avg_rows, dtype=F32)
    rows, total = avg_rows.shape
    e_hi = total if e_hi is None else e_hi
    with _quiet():
        v = avg_rows if adj is None else (avg_rows - np.asarray(adj, dtype=F32)[None, :]).astype(F32)
        v = v.copy()
        v[:, :e_lo] = -np.inf
        v[:, e_hi:] = -np.inf
        out = np.max(v.reshape(rows, width, total // width), axis=2)
    if ring is None:
        return out
    ring = np.array(ring, dtype=F32).copy()
    for p in range(rows):
        ring[(row0 + p) % HM_ROWS] = out[p]
    return ring


def merge_rows(partials):
    """ksa_scan_merge_rows_dev: NaN-propagating maximum of the shards' partial rows ([world][rows][width])."""
    with _quiet():
        return np.max(np.asarray(partials, dtype=F32), axis=0)


# ------------------------------------------------------------------------------------------------ the accumulate launch plan
# run_accumulate (csrc/ksa_api.hip) and accumulate_reduce_kernel (csrc/ksa_kernels.hpp), restated; the host test holds these
# lines against the source text, so a rule that moves is noticed before the GPU cases drift off the chunk boundaries.
CHUNK_RULE_SOURCE = {
    "csrc/ksa_api.hip": (
        "e->max_chunks = (int)std::max<size_t>(1, std::min<size_t>(128, (64u << 20) / (3 * nn * 4)));",
        "int chunks = std::min(e->max_chunks, std::max(1, nframes / 64));",
        "a.chunk = (nframes + chunks - 1) / chunks;",
        "chunks = (nframes + a.chunk - 1) / a.chunk;",
    ),
    "csrc/ksa_kernels.hpp": (
        "const int per = (chunks + 15) / 16;",
        "const float w = e > 160 ? 0.f : ldexpf(1.0f, -(int)e);",
    ),
}


def chunk_plan(nframes, n):
    """(frames per chunk, chunks, chunks per reduce group) of a batch of nframes frames of n bins."""
    max_chunks = max(1, min(128, (64 << 20) // (3 * n * 4)))
    chunks = min(max_chunks, max(1, nframes // 64))
    chunk = -(-nframes // chunks)
    chunks = -(-nframes // chunk)
    return chunk, chunks, (chunks + 15) // 16
