"""The state, plot and stitch kernels of libksa.so on injected data, against tests/state_model.py.

The engine hands out its state pointers (ksa_state_dev, ksa_scan_state_dev) and takes dB rows directly (ksa_scan_stitch_passes_dev,
ksa_scan_stitch_range_dev, ksa_merge_gathered_dev, ksa_frame_spectrum), so these kernels are fed curves, rows and bands chosen
here -- NaN, +-inf, both zeros, ties -- without the transform's fp32 noise in between, at the smallest sizes at which each code
path exists (fft_size 16, window "ones", full_size = fft_size unless a case says otherwise).  Comparisons are exact wherever the
arithmetic is pinned (element-wise float32 chains, maxima, sorts); the two averages carry a bound derived where it is used.
"Exact" compares values and NaN patterns: the sign of a zero that is the maximum of a cell holding both zeros is np.max's choice
in the model and v_max_f32's on the device, and nothing downstream tells the zeros apart.

Every device buffer handed to a `_dev` call is a `Guarded` one (tests/companion_sweep.py): guards on both sides, inputs compared
byte for byte after the call, outputs written only in the ranges the header names.
Soak: KSA_RANDOM_CASES=200 KSA_RANDOM_SEED=7 python -m pytest tests/test_gpu_state_sweep.py -m gpu -q  (five draws per case
instead of one; the seed moves every draw)."""
import math
import os

import numpy as np
import pytest

import kernel_catalogue as kc
import ksa_oracle as orc
import pfb_helper as pfb
import pfbpsd_helper as pp
import state_model as sm
from companion_sweep import GUARD_WORD, Guarded
from test_gpu_kernel_catalogue import expected_path, in_format, stream
from test_gpu_parity import assert_db, assert_lin
from test_gpu_psd import assert_psd

pytestmark = pytest.mark.gpu

COUNT = int(os.environ.get("KSA_RANDOM_CASES", "40"))
SEED = int(os.environ.get("KSA_RANDOM_SEED", "20201226"))
ROUNDS = max(1, COUNT // 40)
F32 = np.float32
U24 = 2.0 ** -24
WORST = {}          # name -> largest error / bound seen (printed by the last test)
SEEN = {}           # name -> cases run


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _note(name, ratio=None, cases=1):
    SEEN[name] = SEEN.get(name, 0) + cases
    if ratio is not None:
        WORST[name] = max(WORST.get(name, 0.0), float(ratio))


def _rngs(*key):
    """One generator per soak round, seeded by KSA_RANDOM_SEED and the case."""
    for r in range(ROUNDS):
        yield np.random.default_rng([SEED, r] + [int(k) for k in key])


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want, equal_nan=True):
        with np.errstate(invalid="ignore"):
            bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))).reshape(-1))
        i = int(bad[0])
        raise AssertionError("%s: %d of %d values differ, the first at %d: %r, not %r" % (
            what, len(bad), got.size, i, got.reshape(-1)[i], want.reshape(-1)[i]))


def _put(torch, view, values):
    """Write a numpy array into library-owned device memory."""
    t = torch.as_tensor(view, device="cuda")
    t.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=F32)).reshape(t.shape).to("cuda"))
    torch.cuda.synchronize()


def _get(torch, view):
    torch.cuda.synchronize()
    return torch.as_tensor(view, device="cuda").cpu().numpy().copy()


def _engine(ksa, n=16, **kw):
    kw.setdefault("full_size", n)
    kw.setdefault("window", "ones")
    kw.setdefault("xres", 4)
    return ksa.SpectrumEngine(n, **kw)


def _scan_engine(ksa, total, width, q=0.5, **kw):
    return _engine(ksa, 16, scan_total_entries=total, scan_non_overlap=q, scan_xres=width, **kw)


def _sprinkle(rng, v, values, share=16):
    """Overwrite about len(v)/share elements (at least one per value where there is room) with each of `values`."""
    for s in values:
        k = max(1, len(v) // share)
        v[rng.choice(len(v), min(k, len(v)), replace=False)] = s
    return v


def _curves(rng, n):
    """cur, max, min, avg: values of both signs; +-0; +inf only; both infinities; everything and NaN."""
    base = [(rng.uniform(-120, 40, n) * rng.choice([1, 1, 1e-3], n)).astype(F32) for _ in range(4)]
    _sprinkle(rng, base[0], [0.0, -0.0], 8)
    _sprinkle(rng, base[1], [np.inf], 32)
    _sprinkle(rng, base[2], [np.inf, -np.inf], 24)
    _sprinkle(rng, base[3], [np.nan, np.inf, -np.inf, 0.0, -0.0], 40)
    return np.array(base, dtype=F32)


# ------------------------------------------------------------------------------------------------ levels
def _avg_within(got, want, state, adj, cells, tag):
    """AVG levels against the model.  levels_kernel adds the g float32 differences one after the other in float64 and divides
    by g.  A sequential float64 sum of g terms is off by at most (g - 1) 2^-53 sum|v| <= (g - 1) g 2^-53 max|v|; divided by g,
    and with the division's own rounding (2^-53 |mean| <= 2^-53 max|v|), the device's float64 mean lies within g 2^-52 max|v|
    of the exact one.  Both are then rounded to float32, which moves each by at most half an ulp and keeps their order: the
    float32 results differ by at most one float32 ulp plus that distance.  Non-finite cells must match exactly."""
    k, n = state.shape
    g = n // cells
    with np.errstate(invalid="ignore"):
        v = (state if adj is None else (state - adj[None, :]).astype(F32)).reshape(k, cells, g)
        fin = np.isfinite(want)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin], want[~fin], equal_nan=True), tag
        top = np.max(np.where(np.isfinite(v), np.abs(v), 0).astype(np.float64), axis=2)
        bound = np.spacing(np.abs(want[fin])).astype(np.float64) + g * 2.0 ** -52 * top[fin]
        err = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64))
    assert np.all(err <= bound), "%s: %g over its bound" % (tag, float(np.max(err / bound)))
    _note("levels AVG", float(np.max(err / bound, initial=0.0)))


def _check_levels(eng, state, adj, cells_list, scan, what):
    for mode in ("AVG", "MAX", "MIN"):
        for cells in cells_list:
            got = eng.levels(cells, mode, scan=scan).astype(F32)
            want = sm.levels(state, adj, cells, mode)
            tag = "%s %s cells %d" % (what, mode, cells)
            if mode != "AVG":
                _same(got, want, tag)
                _note("levels " + mode)
            else:
                _avg_within(got, want, state, adj, cells, tag)


@pytest.mark.parametrize("n", [16, 64, 4096, 1500])
def test_levels_of_injected_zero_span_state(ksa, torch_cuda, n):
    """One cell, g = 1, g = 2, cell counts that are no multiple of the 128-thread block (n = 1500: 125 and 375, n / 2 = 750)."""
    eng = _engine(ksa, n)
    cells = [1, 2, n // 2, n] + ([125, 375] if n == 1500 else [])
    for rng in _rngs(1, n):
        state = _curves(rng, n)
        _put(torch_cuda, eng.state_dev()[0], state)
        adj = _sprinkle(rng, rng.uniform(-3, 3, n).astype(F32), [0.0], 8)
        for a in (None, adj):
            eng.set_adj(a, scan=False)
            _check_levels(eng, state, a, cells, False, "zeroSpan n %d adj %s" % (n, a is not None))
    # +inf and -inf in one cell give NaN, whatever else it holds
    state = np.zeros((4, n), F32)
    state[:, 0], state[:, n - 1] = np.inf, -np.inf
    _put(torch_cuda, eng.state_dev()[0], state)
    eng.set_adj(None, scan=False)
    lv = eng.levels(1, "AVG")
    assert np.isnan(lv).all() and np.all(eng.levels(1, "MAX") == np.inf) and np.all(eng.levels(1, "MIN") == -np.inf)
    eng.close()


@pytest.mark.parametrize("cells", [129, 1023, 1025])
def test_levels_of_injected_scan_state(ksa, torch_cuda, cells):
    """The scan state (its own adj), totals 16 x 129, 16 x 1023, 16 x 1025: g = 16 at an odd cell count either side of 1024."""
    total = 16 * cells
    eng = _scan_engine(ksa, total, cells)
    for rng in _rngs(2, cells):
        state = _curves(rng, total)
        _put(torch_cuda, eng.scan_state_dev()[0], state)
        adj = rng.uniform(-3, 3, total).astype(F32)
        for a in (None, adj):
            eng.set_adj(a, scan=True)
            _check_levels(eng, state, a, [1, cells, total], True, "scan total %d adj %s" % (total, a is not None))
    eng.close()


# ------------------------------------------------------------------------------------------------ highs
SHAPES = ("distinct", "three levels", "all equal", "all NaN", "NaN and +inf", "-inf floor", "both zeros", "plateaus")
MIN_SEPS = (0.0, 0.5, 1.0, 1.5, 7.0, 7.0 - 2.0 ** -40, 7.0 + 2.0 ** -40, "cells", 1e9)
COUNTS = (1, 2, 63, 64)


def _shape(rng, name, cells):
    if name == "distinct":
        return (rng.permutation(cells) * 0.25 - 70).astype(F32)
    if name == "three levels":
        return rng.choice(np.array([-50, -30, -10], F32), cells)
    if name == "all equal":
        return np.full(cells, -42.5, F32)
    if name == "all NaN":
        return np.full(cells, np.nan, F32)
    if name == "NaN and +inf":
        v = (rng.permutation(cells) * 0.25 - 70).astype(F32)
        v[rng.choice(cells, min(cells, 3), replace=False)] = np.nan
        v[rng.integers(0, cells)] = np.inf
        return v
    if name == "-inf floor":
        v = rng.choice(np.array([-50, -30, -10], F32), cells)
        v[rng.random(cells) < 0.5] = -np.inf
        return v
    if name == "plateaus":      # runs of equal cells on a rising ramp with one NaN: ties between neighbours, the highest run last
        v = (np.arange(cells) // 5).astype(F32) - F32(30)
        v[rng.integers(0, cells)] = np.nan
        return v
    assert name == "both zeros"
    return rng.choice(np.array([0.0, -0.0, -1.0, -2.5], F32), cells)


@pytest.mark.parametrize("cells", [1, 2, 3, 64, 1023, 1024, 1025, 4096])
def test_highs_of_injected_curves(ksa, torch_cuda, cells):
    """highs_kernel on curves it is handed as they are (scan state of `cells` elements read at g = 1): indices, levels and
    `found` equal the model.  Up to 64 cells every (count, min_sep) pair runs on every shape; above, every min_sep and every
    count runs on every shape with the other one rotating.  The cases hold found == 0 (one cell), found < count (two and
    three cells, a spacing wider than the curve, all-NaN at count 64) and more cells than the kernel's 1024 threads."""
    eng = _scan_engine(ksa, cells, 1)
    short, none = 0, 0
    for rng in _rngs(3, cells):
        for half in (0, 4):
            state = np.array([_shape(rng, s, cells) for s in SHAPES[half:half + 4]])
            _put(torch_cuda, eng.scan_state_dev()[0], state)
            for c, name in enumerate(SHAPES[half:half + 4]):
                if cells <= 64:
                    pairs = [(k, s) for k in COUNTS for s in MIN_SEPS]
                else:
                    pairs = [(COUNTS[(i + c) % 4], s) for i, s in enumerate(MIN_SEPS)] + [(k, MIN_SEPS[(2 * i + c) % 9]) for i, k in enumerate(COUNTS)]
                for count, sep in pairs:
                    sep = float(cells) if sep == "cells" else sep
                    idx, lvl = eng.highs(cells, "MAX", ("cur", "max", "min", "avg")[c], min_sep=sep, count=count, scan=True)
                    marks, want, found = sm.highs(state[c], sep, count)
                    tag = "%s, %d cells, count %d, min_sep %r" % (name, cells, count, sep)
                    assert list(idx) == marks, "%s: cells %s, not %s" % (tag, list(idx)[:8], marks[:8])
                    _same(lvl.astype(F32), np.array(want, F32), tag + " levels")
                    short += found < count
                    none += found == 0
                    _note("highs")
    assert short > 0 and (none > 0) == (cells == 1)
    eng.close()


# ------------------------------------------------------------------------------------------------ view
def test_view_equals_the_separate_calls_and_the_model(ksa, torch_cuda):
    """ksa_read_view after set_hm_index at 0, 1 and 127 with 0, 1, 127 and 128 rows: levels, markers, rows (oldest first, across
    the wrap) and hm_index equal ksa_read_levels / ksa_read_highs / ksa_read_hm_rows and the model."""
    n, w = 64, 16
    eng = _engine(ksa, n, xres=w)
    for rng in _rngs(4):
        state = _curves(rng, n)
        ring = rng.normal(size=(128, w)).astype(F32)
        ring[5, 3] = np.nan
        _put(torch_cuda, eng.state_dev()[0], state)
        _put(torch_cuda, eng.state_dev()[1], ring)
        adj = rng.uniform(-3, 3, n).astype(F32)
        eng.set_adj(adj, scan=False)
        for idx in (0, 1, 127):
            eng.set_hm_index(idx)
            for rows in (0, 1, 127, 128):
                for mode, curve, cells in (("MAX", "max", 16), ("AVG", "cur", 32), ("MIN", "avg", 64)):
                    cv = ("cur", "max", "min", "avg").index(curve)
                    lv, marks, lvl, got_rows, got_idx = eng.view(cells, mode, curve, min_sep=1.5, count=5, hm_rows=rows)
                    want = sm.view(state, adj, ring, idx, cells, mode, cv, 1.5, 5, rows)
                    if mode != "AVG":
                        _same(lv.astype(F32), want[0], "view levels")
                        assert list(marks) == want[1], "view markers against the model"
                        _same(lvl.astype(F32), np.array(want[2], F32), "view marker levels against the model")
                    else:       # (an AVG level may sit an ulp off the model's: the markers are the model's walk over the device's levels)
                        _avg_within(lv.astype(F32), want[0], state, adj, cells, "view AVG levels")
                        walk = sm.highs(lv[cv].astype(F32), 1.5, 5)
                        assert list(marks) == walk[0], "view markers against the model's walk"
                        _same(lvl.astype(F32), np.array(walk[1], F32), "view marker levels against the model's walk")
                    _same(lv, eng.levels(cells, mode), "view levels vs ksa_read_levels")
                    i2, l2 = eng.highs(cells, mode, curve, min_sep=1.5, count=5)
                    assert list(marks) == list(i2)
                    _same(lvl, l2, "view marker levels vs ksa_read_highs")
                    _same(got_rows.astype(F32), want[4], "view rows idx %d rows %d" % (idx, rows))
                    if rows:
                        _same(got_rows, eng.hm_rows(idx - rows, rows), "view rows vs ksa_read_hm_rows")
                    assert got_idx == idx
                    _note("view")
    eng.close()


def test_view_of_the_scan_state(ksa, torch_cuda):
    """The same on the scan state: three one-pass stitches move its ring position to 3 (rowmax_kernel writes the rows), then
    state and ring are injected."""
    torch = torch_cuda
    total, w = 16 * 129, 129
    eng = _scan_engine(ksa, total, w)
    nsteps = total // 8
    rng = next(_rngs(5))
    # what fill_kernel wrote at creation (K:603-608, K:613-614): Cur = Max = Avg = dB(minAmp4Clip), Min = dB(1.0), ring = minAmp4Clip
    st = eng.scan_state()
    floor = F32(10.0 * math.log10(float(F32(eng.min_amp))) - float(F32(eng.gain)))
    for key, v in (("Fft.Cur", floor), ("Fft.Max", floor), ("Fft.Avg", floor), ("Fft.Min", F32(-float(F32(eng.gain))))):
        _same(st[key].astype(F32), np.full(total, v, F32), "fresh scan state " + key)
    _same(st["fftHM"].astype(F32), np.full((128, w), F32(eng.min_amp)), "fresh scan ring")
    for p in range(3):
        bands = Guarded.input(torch, rng.normal(size=(nsteps, 16)).astype(F32), name="step_db")
        eng.scan_stitch_dev(bands.ptr, nsteps)
        eng.synchronize()
        bands.check()
        st = eng.scan_state()
        assert st["hm_index"] == p + 1 and st["passes"] == p + 1
        _same(st["fftHM"][p].astype(F32), sm.scan_rows(st["Fft.Avg"].astype(F32)[None, :], None, w, 0)[0], "row of pass %d" % p)
    state = _curves(rng, total)
    ring = rng.normal(size=(128, w)).astype(F32)
    _put(torch, eng.scan_state_dev()[0], state)
    _put(torch, eng.scan_state_dev()[1], ring)
    for rows in (0, 1, 4, 128):
        lv, marks, lvl, got_rows, got_idx = eng.view(w, "MAX", "avg", min_sep=7.0, count=64, hm_rows=rows, scan=True)
        want = sm.view(state, None, ring, 3, w, "MAX", 3, 7.0, 64, rows)
        _same(lv.astype(F32), want[0], "scan view levels")
        assert list(marks) == want[1] and got_idx == 3
        _same(lvl.astype(F32), np.array(want[2], F32), "scan view marker levels")
        _same(got_rows.astype(F32), want[4], "scan view rows %d" % rows)
        _note("view")
    eng.close()


# ------------------------------------------------------------------------------------------------ frame_spectrum
@pytest.mark.parametrize("n", [16, 256, 512, 16384, 65536])
@pytest.mark.parametrize("cell", ["1", "4", "n/4"])
def test_frame_spectrum_rows_state_and_ring(ksa, torch_cuda, n, cell):
    """db_rows_kernel: one block below 256 bins, one, two, and the 64-block grid-stride loop at 65536; waterfall cells of 1, 4
    and n/4 bins; three calls whose rows wrap ring slot 127 -> 0 -> 1, the second and third with a baseline.  Magnitudes hold
    0 (-inf dB), NaN, +inf and one denormal, which the hardware logarithm reads as zero (ksa.h: ksa_frame_spectrum).  The dB row
    (Fft.Cur after the call) is held against the float64 model with assert_db; everything derived from it (ring row, Max,
    Min, Avg) against the device's own row, exactly: one commit of one frame is a * 2^-1 + x * 2^-1 rounded once, which is the
    correctly rounded (a + x) / 2 of the model."""
    g = {"1": 1, "4": 4, "n/4": n // 4}[cell]
    w = n // g
    eng = _engine(ksa, n, xres=w, gain=19.1)
    assert eng.hm_width == w
    rng = next(_rngs(6, n, g))
    eng.set_hm_index(127)
    ring = eng.state()["fftHM"].astype(F32)
    state, has, adj = None, (0, 0, 0), None
    for call in range(3):
        mag = (10.0 ** rng.uniform(-6, 1, n)).astype(F32)
        mag[rng.choice(n, 4, replace=False)] = [0.0, np.nan, np.inf, 1e-40]
        tiny = mag == F32(1e-40)
        if call == 1:
            adj = rng.uniform(-3, 3, n).astype(F32)
            eng.set_adj(adj, scan=False)
        eng.frame_spectrum(mag)
        st = eng.state()
        cur = st["Fft.Cur"].astype(F32)
        db, _ = sm.db_rows(mag, 19.1, None, 0)
        assert np.all(np.isneginf(cur[tiny])), "the denormal magnitude did not read as zero"
        db[tiny] = -np.inf
        assert np.array_equal(np.isneginf(cur), np.isneginf(db)) and np.array_equal(np.isnan(cur), np.isnan(db))
        assert np.array_equal(np.isposinf(cur), np.isposinf(db))
        assert_db(np.where(np.isposinf(cur), 0, cur), np.where(np.isposinf(db), 0, db), what="frame_spectrum n %d call %d" % (n, call))
        state, has = sm.accumulate(cur[None, :], 0, 1, state, has, (1, 1, 1))
        for c, k in enumerate(("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg")):
            _same(st[k].astype(F32), state[c].astype(F32), "frame_spectrum n %d call %d %s" % (n, call, k))
        state = np.array([st[k] for k in ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg")])
        ring = sm.scan_rows(cur[None, :], adj, w, (127 + call) % 128, ring=ring)
        _same(st["fftHM"].astype(F32), ring, "frame_spectrum n %d call %d ring" % (n, call))
        assert st["hm_index"] == (128 + call) % 128 and st["frames"] == call + 1
        _note("frame_spectrum")
    eng.close()


# ------------------------------------------------------------------------------------------------ accumulate
ACC_COUNTS = [1, 63, 64, 127, 128, 129, 161, 1087, 1088, 1089, 8191, 8192, 8193]


def _special_frames(k):
    """Frames that get a special block: the first and the last, and either side of every chunk boundary of the launch plan."""
    chunk, chunks, _ = sm.chunk_plan(k, 16)
    at = {0, k - 1}
    for c in range(1, chunks):
        at |= {c * chunk - 1, c * chunk}
    return sorted(f for f in at if 0 <= f < k)


def _acc_iq(rng, k, variant):
    """k blocks of 16 complex samples, noise at three levels.  "plain": nothing else (every bin of Avg stays finite).  Special
    blocks (see _special_frames) are, by the other variants: "lines" blocks of period 2 or 4
    (a + b (-1)^t + c i^t + d (-i)^t), whose spectrum is zero (-inf dB where the transform cancels exactly) outside two to four
    bins and never zero at DC and Nyquist, so that those two bins stay finite through the whole run; "zeros" all-zero blocks
    (-inf rows); "nan" all-zero blocks and blocks with one NaN sample, alternating."""
    x = (rng.normal(size=(k, 16)) + 1j * rng.normal(size=(k, 16))).astype(np.complex64) * rng.choice([0.01, 0.3, 1.0], (k, 1)).astype(F32)
    t = np.arange(16)
    alt, quarter = (-1.0) ** t, np.array([1, 1j, -1, -1j])[t % 4]
    lines = (1.0 + 0.5 * alt, 0.75 - 0.25 * alt + 0.25 * quarter, 0.5 + alt + 0.125 * quarter.conj(),
             0.25 + 0.5 * alt + 0.25 * quarter + 0.125 * quarter.conj())
    for j, f in enumerate(_special_frames(k) if variant != "plain" else ()):
        if variant == "lines":
            x[f] = lines[j % 4]
        elif variant == "zeros" or j % 2 == 0:
            x[f] = 0
        else:
            x[f, int(rng.integers(0, 16))] = np.nan
    return x


def _acc_bound(rows, first_index, total, k_chunk, per, prev_avg, seeded):
    """Forward bound of the device's Avg against the exact weighted sum S = sum_f w_f x_f (+ prev 2^-total).
    accumulate_partial_kernel adds the exact products w_f x_f (w_f a power of two) of a chunk one after the other: a term
    takes part in at most chunk - 1 rounded additions (the first lands in a zero).  accumulate_reduce_kernel adds the `per`
    partials of a group the same way (per - 1 more), then the 16 groups through LDS (15 more), and commit_kernel adds
    prev 2^-total (1 more).  For ANY order of additions in which no term passes through more than h of them, the error is at
    most gamma_h sum|terms|, gamma_h = h u / (1 - h u), u = 2^-24 (Higham, Accuracy and Stability, section 4.2).  On top: a
    product below 2^-126 may lose up to 2^-126 (flushed or denormal) -- k 2^-126 in all; the weights the kernel cuts off
    (e > 160) are below 2^-160 max|x|; and the float64 recursion of the model itself is exact to 2^-50 of the same sum."""
    h = (k_chunk - 1) + (per - 1) + 15 + 1
    gamma = h * U24 / (1 - h * U24)
    k, n = rows.shape
    e = total - (first_index + np.arange(k))
    if seeded:
        e[0] = total - 1
    wsum = np.zeros(n)
    fin = np.abs(rows.astype(np.float64))
    fin[~np.isfinite(fin)] = 0
    for f in range(k):
        if e[f] < 1070:
            wsum += 2.0 ** -float(e[f]) * fin[f]
    if prev_avg is not None and total < 1070:
        wsum += 2.0 ** -float(total) * np.where(np.isfinite(prev_avg), np.abs(prev_avg), 0)
    return (gamma + 2.0 ** -50) * wsum + k * 2.0 ** -126 + 2.0 ** -159 * np.max(fin, initial=0.0)


def _check_state(st, want, bound, what):
    for c, key in enumerate(("Fft.Cur", "Fft.Max", "Fft.Min")):
        _same(st[key], want[c], what + " " + key)
    avg, ref = st["Fft.Avg"], want[3]
    assert np.array_equal(np.isnan(avg), np.isnan(ref)) and np.array_equal(np.isneginf(avg), np.isneginf(ref)), what + ": NaN / -inf pattern of Avg"
    assert np.array_equal(np.isposinf(avg), np.isposinf(ref)), what + ": +inf pattern of Avg"
    fin = np.isfinite(ref)
    ratio = np.max(np.abs(avg[fin] - ref[fin]) / bound[fin], initial=0.0)
    print("%s: Avg error / bound %.3g" % (what, ratio))
    assert ratio <= 1.0, "%s: Avg is %.3g times its bound off the model" % (what, ratio)
    _note("accumulate", ratio)


def _frames(torch, eng, x, **kw):
    """frames_dev on Guarded buffers: the blocks of x at frame_stride 16 from an address that is sample-aligned only; returns
    the device's dB rows."""
    k = len(x)
    iq = Guarded.input(torch, x, misalign=8, name="iq")
    db = Guarded.output(torch, k * 16 * 4, name="cur_db").own(0, k * 16 * 4)
    eng.frames_dev(iq.ptr, 0, k, cur_db=db.ptr, frame_stride=16, **kw)
    eng.synchronize()
    iq.check()
    db.check()
    return db.read(F32).reshape(k, 16)


@pytest.mark.parametrize("variant", ["plain", "lines", "zeros", "nan"])
@pytest.mark.parametrize("k", ACC_COUNTS)
def test_accumulate_counts_around_the_launch_plan(ksa, torch_cuda, k, variant):
    """accumulate_partial_kernel / accumulate_reduce_kernel / commit_kernel: one chunk, two chunks (128 frames on), the weight
    cut-off (beyond 160 frames), more than one partial per reduce group (1088 frames on) and the largest chunk counts (127 and
    128 at 8191 .. 8193), with special blocks at the first and last frame and either side of every chunk boundary.  The model
    runs on the device's own dB rows."""
    chunk, chunks, per = sm.chunk_plan(k, 16)
    eng = _engine(ksa, 16, max_frames=k)
    for rng in _rngs(7, k, ("plain", "lines", "zeros", "nan").index(variant)):
        eng.reset()
        rows = _frames(torch_cuda, eng, _acc_iq(rng, k, variant))
        if variant != "nan":
            assert not np.isnan(rows).any()
        if variant == "plain":
            assert np.isfinite(rows).all()
        if variant == "lines":
            assert np.isneginf(rows).any() and np.isfinite(rows).all(axis=0).any(), "the special blocks do not do what they are for"
        want, _ = sm.accumulate(rows, 0, k, None, (0, 0, 0), (1, 1, 1))
        st = eng.state()
        _check_state(st, want, _acc_bound(rows, 0, k, chunk, per, None, True), "accumulate %d frames (%s)" % (k, variant))
        assert st["frames"] == k and st["hm_index"] == k % 128
    eng.close()


def test_accumulate_where_max_chunks_sets_the_chunk_count(ksa, torch_cuda):
    """n = 65536, 5505 frames at frame_stride 16: run_accumulate's max_chunks is 85 at this size, below nframes / 64 = 86, so
    the chunks are 65 frames long and the reduce groups fold six partials each.  The dB rows are 1.4 GB: every 61st bin is
    gathered on the device before the read-back.  61 is odd and no multiple of 4, so the sampled bins fall on every position
    inside the 4-bin threads of accumulate_partial_kernel and inside the 64-bin workgroups of accumulate_reduce_kernel.  The
    whole payload of cur_db is owned by the call, so only its guards are compared (check() would bring it to the host)."""
    torch = torch_cuda
    n, k, step = 65536, 5505, 61
    chunk, chunks, per = sm.chunk_plan(k, n)
    assert (chunk, chunks, per) == (65, 85, 6) and chunks < k // 64
    eng = _engine(ksa, n, max_frames=k, xres=64)
    rng = next(_rngs(14))
    x = (rng.normal(size=(k - 1) * 16 + n) + 1j * rng.normal(size=(k - 1) * 16 + n)).astype(np.complex64)
    iq = Guarded.input(torch, x, misalign=8, name="iq")
    db = Guarded(torch, k * n * 4, name="cur_db")
    eng.frames_dev(iq.ptr, 0, k, cur_db=db.ptr, frame_stride=16)
    eng.synchronize()
    iq.check()
    end = db.start + db.nbytes
    for lo, hi, what in ((0, db.start, "before"), (end, len(db.buf), "after")):
        guard = np.frombuffer((GUARD_WORD * ((hi - lo) // 4 + 1))[:hi - lo], dtype=np.uint8)
        assert np.array_equal(db.buf[lo:hi].cpu().numpy(), guard), "cur_db: the guard %s the payload was written" % what
    rows = db.payload.view(torch.float32).reshape(k, n)[:, ::step].contiguous().cpu().numpy()
    assert np.isfinite(rows).all()
    want, _ = sm.accumulate(rows, 0, k, None, (0, 0, 0), (1, 1, 1))
    full = eng.state()
    st = {key: full[key][::step] for key in ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg")}
    _check_state(st, want, _acc_bound(rows, 0, k, chunk, per, None, True), "accumulate %d frames of %d bins" % (k, n))
    assert full["frames"] == k
    eng.close()


@pytest.mark.parametrize("k", ACC_COUNTS[1:])
def test_accumulate_split_runs(ksa, torch_cuda, k):
    """The same counts split at a third: (a) the two batches as shards of one run (first_index / total_frames, commit = 0),
    their partial blocks [max | cur | -min | sum] merged the way the header tells an all-reduce to (MAX of rows 0-2, SUM of row
    3), put back and committed; (b) as two committed batches, the second on top of the first (has_prev)."""
    torch = torch_cuda
    k1 = (k + 1) // 3
    k2 = k - k1
    eng = _engine(ksa, 16, max_frames=k)
    rng = next(_rngs(8, k))
    x = _acc_iq(rng, k, "lines")
    # (a)
    parts, rows = [], []
    for lo, cnt in ((0, k1), (k1, k2)):
        rows.append(_frames(torch, eng, x[lo:lo + cnt], first_index=lo, total_frames=k, commit=False))
        parts.append(_get(torch, eng.partial()))
    assert np.all(np.isneginf(parts[0][1])), "a batch that does not own the run's last frame must leave cur at -inf"
    _same(parts[1][1], rows[1][-1], "cur of the batch that owns the last frame")
    merged = np.concatenate([sm.nan_max(parts[0][:3], parts[1][:3]), (parts[0][3:] + parts[1][3:]).astype(F32)])
    _put(torch, eng.partial(), merged)
    eng.commit(k)
    allrows = np.concatenate(rows)
    want, _ = sm.accumulate(allrows, 0, k, None, (0, 0, 0), (1, 1, 1))
    ca, _, pa = sm.chunk_plan(k1, 16)
    cb, _, pb = sm.chunk_plan(k2, 16)
    bound = _acc_bound(allrows, 0, k, max(ca, cb) + 1, max(pa, pb), None, True)          # (+ 1: the merge's own addition)
    _check_state(eng.state(), want, bound, "accumulate %d frames as two shards" % k)
    # (b)
    eng.reset()
    r1 = _frames(torch, eng, x[:k1])
    w1, has = sm.accumulate(r1, 0, k1, None, (0, 0, 0), (1, 1, 1))
    s1 = eng.state()
    b1 = _acc_bound(r1, 0, k1, ca, pa, None, True)
    _check_state(s1, w1, b1, "accumulate %d frames, first batch of %d" % (k, k1))
    r2 = _frames(torch, eng, x[k1:])
    prev = np.array([s1[key] for key in ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg")])   # (the device's own first state: its error is not carried)
    w2, _ = sm.accumulate(r2, 0, k2, prev, has, (1, 1, 1))
    _check_state(eng.state(), w2, _acc_bound(r2, 0, k2, cb, pb, prev[3], False), "accumulate %d frames, second batch of %d" % (k, k2))
    assert eng.state()["frames"] == k
    eng.close()


@pytest.mark.parametrize("flags", range(8))
def test_accumulate_flags_toggled_between_batches(ksa, torch_cuda, flags):
    """bDataMax / bDataMin / bDataAvg in one of the eight combinations for a first batch of 129 frames, the complement for a
    second, all on for a third: a curve is seeded by copy the first time its flag is on and left alone while it is off."""
    k = 129
    chunk, _, per = sm.chunk_plan(k, 16)
    first = tuple(bool(flags >> b & 1) for b in range(3))
    eng = _engine(ksa, 16, max_frames=k)
    rng = next(_rngs(9, flags))
    state, has = None, (0, 0, 0)
    for batch, fl in enumerate((first, tuple(not f for f in first), (True, True, True))):
        eng.set_flags(*fl)
        rows = _frames(torch_cuda, eng, _acc_iq(rng, k, "lines"))
        had_avg = has[2]
        want, has = sm.accumulate(rows, 0, k, state, has, fl)
        st = eng.state()
        bound = _acc_bound(rows, 0, k, chunk, per, state[3] if (state is not None and had_avg) else None, not had_avg)
        _check_state(st, want, bound, "flags %s batch %d" % (fl, batch))
        state = np.array([st[key] for key in ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg")])
    eng.close()


# ------------------------------------------------------------------------------------------------ merge_gathered
@pytest.mark.parametrize("width", [4, 16])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_merge_gathered_blocks_of_its_own_choosing(ksa, torch_cuda, world, width):
    """merge_gathered_kernel on random exchange blocks with NaN: frames per rank 1, 5, 127, 128, 129, 300 x ring position 0, 1,
    127.  A matching frames_dev(commit = 0) makes the frames pending (and writes this engine's own ring rows, which every
    mapped row of the gathered blocks then replaces).  State and ring on a fresh engine equal the model exactly, the sum
    included: the kernel only adds there, in rank order."""
    torch = torch_cuda
    n = 16
    eng = _engine(ksa, n, xres=width, max_frames=300)
    for rng in _rngs(10, world, width):
        for fpr in (1, 5, 127, 128, 129, 300):
            for idx0 in (0, 1, 127):
                eng.reset()
                eng.set_hm_index(idx0)
                x = (rng.normal(size=(fpr, 16)) + 1j * rng.normal(size=(fpr, 16))).astype(np.complex64)
                _frames(torch, eng, x, first_index=0, total_frames=world * fpr, commit=False)
                ring0 = eng.state()["fftHM"].astype(F32)
                blocks = (rng.normal(size=(world, 4 * n + 128 * width)) * 30).astype(F32)
                _sprinkle(rng, blocks.reshape(-1), [np.nan, -np.inf, 0.0, -0.0], 64)
                gathered = Guarded.input(torch, blocks, name="gathered")
                eng.merge_gathered(gathered.ptr, world, fpr, idx0)
                eng.synchronize()
                gathered.check()
                part, ring = sm.merge_gathered(blocks, world, fpr, idx0, width, ring0)
                st = eng.state()
                tag = "merge world %d fpr %d idx0 %d width %d" % (world, fpr, idx0, width)
                _same(_get(torch, eng.partial()), part, tag + " partial")
                want = sm.commit_fresh(part)
                for c, key in enumerate(("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg")):
                    _same(st[key].astype(F32), want[c], tag + " " + key)
                _same(st["fftHM"].astype(F32), ring, tag + " ring")
                assert st["hm_index"] == (idx0 + world * fpr) % 128 and st["frames"] == world * fpr
                _note("merge_gathered")
    eng.close()


# ------------------------------------------------------------------------------------------------ stitch
HOPS = {1.0: 16, 0.75: 12, 0.5: 8, 0.3125: 5, 0.25: 4, 0.125: 2}      # scan_non_overlap -> hop: one to eight covering bands
SENTINEL = F32(-12345.5)                                              # (no dB band or row of these tests holds it)
PASSES = (1, 2, 31, 32, 33, 64, 65)                                   # around the kernel's groups of AHEAD = 32 passes
GEOMETRY = ((64, 64), (64, 32), (64, 4), (2080, 16))                  # (total, waterfall width): g = 1, 2, 16 and 130 (> 64 lanes)


def _bands(rng, npasses, nsteps):
    b = (rng.normal(size=(npasses, nsteps, 16)) * 20 - 60).astype(F32)
    _sprinkle(rng, b.reshape(-1), [np.nan, np.inf, -np.inf, 0.0], 97)
    return b


def _stitch_case(torch, ksa, rng, q, npasses, total, width, base_is_raw, with_adj):
    hop = HOPS[q]
    nsteps = -(-total // hop)
    eng = _scan_engine(ksa, total, width, q=q)
    eng.scan_set_base_is_raw(base_is_raw)
    adj = rng.uniform(-3, 3, total).astype(F32) if with_adj else None
    eng.set_adj(adj, scan=True)
    state = (rng.normal(size=(4, total)) * 20 - 60).astype(F32)
    state[:, int(rng.integers(0, total))] = np.nan
    _put(torch, eng.scan_state_dev()[0], state)
    ring = eng.scan_state()["fftHM"].astype(F32)
    idx, done = 0, 0
    for call in range(2):          # a first call (pass 0 seeds Avg by copy) and one on top of the state it left
        bands = _bands(rng, npasses, nsteps)
        dev = Guarded.input(torch, bands, name="step_db")
        eng.scan_stitch_dev(dev.ptr, nsteps, npasses)
        eng.synchronize()
        dev.check()
        state, avg_rows = sm.stitch(bands, 16, hop, total, state, call == 0, base_is_raw)
        rows = min(npasses, 128)
        ring = sm.scan_rows(avg_rows[-rows:], adj, width, (idx + npasses - rows) % 128, ring=ring)
        idx, done = (idx + npasses) % 128, done + npasses
        st = eng.scan_state()
        tag = "stitch hop %d, %d passes, total %d, width %d, raw %d, call %d" % (hop, npasses, total, width, base_is_raw, call)
        for c, key in enumerate(("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg")):
            _same(st[key].astype(F32), state[c], tag + " " + key)
        _same(st["fftHM"].astype(F32), ring, tag + " ring")
        assert st["hm_index"] == idx and st["passes"] == done, tag
        _note("stitch")
    eng.close()


@pytest.mark.parametrize("npasses", PASSES)
@pytest.mark.parametrize("q", sorted(HOPS))
def test_stitch_of_injected_bands(ksa, torch_cuda, q, npasses):
    """scan_stitch_kernel + rowmax_kernel (one pass) / rowmax_rows_kernel (a batch) fed dB bands holding NaN, +-inf and +0.0:
    state, ring and ring position bit for bit, with both bScanRangeBaseDataIsRaw values, with and without a scan baseline,
    waterfall cells of 1, 2 and 16 elements."""
    case = sorted(HOPS).index(q) * len(PASSES) + PASSES.index(npasses)
    for rng in _rngs(11, case):
        for raw in (False, True):
            total, width = GEOMETRY[(case + raw) % 3]
            _stitch_case(torch_cuda, ksa, rng, q, npasses, total, width, raw, (case + raw) % 2 == 0)


@pytest.mark.parametrize("q,npasses,raw", [(0.5, 33, False), (0.3125, 65, True), (0.125, 2, False), (1.0, 130, False)])
def test_stitch_with_cells_wider_than_a_wave(ksa, torch_cuda, q, npasses, raw):
    """2080 elements in 16 cells of 130: rowmax_rows_kernel's lanes take more than one element each; 130 passes wrap the ring."""
    _stitch_case(torch_cuda, ksa, next(_rngs(12, npasses)), q, npasses, 2080, 16, raw, True)


@pytest.mark.parametrize("band_major", [False, True])
@pytest.mark.parametrize("world", [2, 3, 5])
@pytest.mark.parametrize("q,total,npasses", [(1.0, 64, 2), (0.5, 64, 33), (0.3125, 64, 2), (0.125, 32, 33), (0.125, 64, 130)])
def test_stitch_shards_equal_one_engine(ksa, torch_cuda, q, total, npasses, world, band_major):
    """The same bands through 2, 3 and 5 shards on one device (scan_shard, band-major halo blocks, scan_rows, scan_merge_rows,
    both layouts of the own block): every shard's slice of the curves, the merged ring and the ring position equal one
    engine's bit for bit, the partial rows equal the model's (-inf where a shard owns nothing of a cell), and elements a shard
    does not own keep their value.  At hop 2 the halo wants 7 bands: more than the 3 to 7 a shard owns."""
    torch = torch_cuda
    hop, width = HOPS[q], 8
    nsteps = -(-total // hop)
    rng = next(_rngs(13, int(q * 1000), total, npasses, world))
    raw = bool((world + npasses) % 2)
    adj = rng.uniform(-3, 3, total).astype(F32)
    state0 = (rng.normal(size=(4, total)) * 20 - 60).astype(F32)
    engines = [_scan_engine(ksa, total, width, q=q) for _ in range(world + 1)]
    one, ranks = engines[0], engines[1:]
    scratch = []
    for e in ranks:
        # the partial rows live in engine scratch of 128 rows: a call that owns nothing makes the engine allocate it, its rows
        # are then set to a value no row can hold, and scan_reset() takes the call back (passes, pending rows) before the state goes in
        e.scan_stitch_range_dev(None, None, 0, 0, 0, nsteps, 1, 0, 0)
        view = e.scan_rows()
        whole = type(view)(view.__cuda_array_interface__["data"][0], (128, width), e)
        _put(torch, whole, np.full((128, width), SENTINEL, F32))
        e.scan_reset()
        scratch.append(whole)
    for e in engines:
        e.scan_set_base_is_raw(raw)
        e.set_adj(adj, scan=True)
        _put(torch, e.scan_state_dev()[0], state0)
    bands = _bands(rng, npasses, nsteps)
    dev = Guarded.input(torch, bands, name="step_db")
    one.scan_stitch_dev(dev.ptr, nsteps, npasses)
    one.synchronize()
    dev.check()
    want = one.scan_state()
    model, avg_rows = sm.stitch(bands, 16, hop, total, state0, True, raw)
    _same(want["Fft.Avg"].astype(F32), model[3], "one engine against the model")
    rows = min(npasses, 128)
    partials, keep = [], []
    for r, e in enumerate(ranks):
        lo, hi, nhalo, e_lo, e_hi = e.scan_shard(nsteps, r, world)
        own = bands[:, lo:hi]
        own = np.ascontiguousarray(own.transpose(1, 0, 2) if band_major else own)
        halo = np.ascontiguousarray(bands[:, lo - nhalo:lo].transpose(1, 0, 2))          # [nhalo][npasses][16]
        g_own = Guarded.input(torch, own, name="own_db") if hi > lo else None
        g_halo = Guarded.input(torch, halo, name="halo_db") if nhalo else None
        e.scan_stitch_range_dev(g_own.ptr if g_own else None, g_halo.ptr if g_halo else None, nhalo, lo, hi, nsteps, npasses,
                                e_lo, e_hi, own_band_major=band_major)
        e.synchronize()
        keep += [g_own, g_halo]
        for gbuf in (g_own, g_halo):
            if gbuf:
                gbuf.check()
        part = _get(torch, e.scan_rows())
        assert part.shape == (rows, width)
        whole = _get(torch, scratch[r])
        _same(whole[:rows], part, "the view is the head of the scratch")
        assert np.all(whole[rows:] == SENTINEL), "shard %d of %d: scratch rows beyond the batch's %d were written" % (r, world, rows)
        _same(part, sm.scan_rows(avg_rows[-rows:], adj, width, 0, e_lo=e_lo, e_hi=e_hi), "partial rows of shard %d of %d" % (r, world))
        partials.append(part)
        st = e.scan_state()
        for c, key in enumerate(("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg")):
            _same(st[key][e_lo:e_hi], want[key][e_lo:e_hi], "shard %d of %d %s" % (r, world, key))
            _same(st[key][:e_lo].astype(F32), state0[c][:e_lo], "shard %d of %d %s in front of its elements" % (r, world, key))
            _same(st[key][e_hi:].astype(F32), state0[c][e_hi:], "shard %d of %d %s behind its elements" % (r, world, key))
    gathered = Guarded.input(torch, np.array(partials, F32), name="gathered rows")
    for r, e in enumerate(ranks):
        e.scan_merge_rows(gathered.ptr, world, rows, npasses)
        e.synchronize()
        st = e.scan_state()
        _same(st["fftHM"], want["fftHM"], "merged ring of shard %d of %d" % (r, world))
        assert st["hm_index"] == want["hm_index"] == npasses % 128 and st["passes"] == npasses
    gathered.check()
    _note("stitch shards")
    for e in engines:
        e.close()


# ------------------------------------------------------------------------------------------------ spectrum-stage buffers
PLANS = ("n16", "n64", "pair", "n2048 split", "n8192", "n32768", "n20", "pfb", "pfbpsd")


def _plan(ksa, plan, frames_of):
    """(engine keywords, frames, frame stride, oracle of one block, expected path, fold) of one launch plan."""
    if plan == "pfb":
        taps = pfb.prototype(16, 4, "hamming")
        return dict(n=16, pfb_taps=4, window=taps, xres=4), 5, 16, lambda b: pfb.spectrum(b, 16, taps), 0, "AVG"
    if plan == "pfbpsd":
        taps = pfb.prototype(16, 4, "hamming")
        return dict(n=16, pfb_taps=4, pfb_spectra=3, window=taps, xres=4), 5, 48, lambda b: pp.spectrum(b, 16, taps), 0, "PSD"
    n = {"n16": 16, "n64": 64, "pair": 1024, "n2048 split": 2048, "n8192": 8192, "n32768": 32768, "n20": 20}[plan]
    q, full = 0.5, 3 * n                                      # five windows per block
    win = orc.window_table("hanning", n)
    kw = dict(n=n, full_size=full, non_overlap=q, window="hanning", xres=min(n, 64) if n != 20 else 4)
    frames, stride = {"pair": (frames_of, 64), "n8192": (2, full), "n32768": (2, full)}.get(plan, (3, full))
    return kw, frames, stride, lambda b: orc.curscan(b, n, q, win, "AVG"), expected_path(n), "AVG"


@pytest.mark.parametrize("fmt", kc.FMTS, ids=lambda f: kc.FMT_NAMES[f])
@pytest.mark.parametrize("plan", PLANS)
def test_spectrum_stage_buffers(ksa, torch_cuda, plan, fmt):
    """One case per launch plan of the spectrum stage and per sample format: the IQ payload at an address that is
    sample-aligned only, in the middle of an allocation (never against its end: an over-read must not become a fault here, it
    shows as a wrong value or not at all); `out`, `cur_db` and `hm_rows` two rows larger than the batch.  The inputs come back
    bit-identical, the outputs are written in [frames][N] and [frames][W] only, and the values are the oracle's (assert_lin /
    assert_db / assert_psd), so the case is not vacuous.  The waterfall rows must be the cell maxima of the device's own dB
    rows, exactly ("n2048 split": three frames are window-split, the rows come from rowmax_batch)."""
    torch = torch_cuda
    frames_of = None
    if plan == "pair":
        probe = ksa.SpectrumEngine(1024, full_size=3072, non_overlap=0.5, window="hanning", xres=64)
        frames_of = 2 * probe.kernel_info()["grid"] + 1       # launch_spec_t pairs from 2 * grid frames up
        probe.close()
    kw, frames, stride, oracle, path, fold = _plan(ksa, plan, frames_of)
    n = kw.pop("n")
    eng = ksa.SpectrumEngine(n, max_frames=frames + 2, **kw)
    info = eng.kernel_info()
    assert info["path"] == path, (plan, info)
    # kernel_info() shows threads, LDS, VGPRs, grid and path only.  What else identifies a plan is asserted from the engine's
    # geometry and the launch rule; that the polyphase folds ran shows in the values (a plain 16-point engine fails their oracle).
    if plan == "pair":
        assert frames >= 2 * info["grid"] and n == 1024          # launch_spec_t: two frames per workgroup from 2 * grid frames up
    elif plan == "pfb":
        assert (eng.pfb_taps, eng.pfb_spectra, eng.full_size) == (4, 0, 64) and np.array_equal(eng.starts, 16 * np.arange(4))
    elif plan == "pfbpsd":
        assert (eng.pfb_taps, eng.pfb_spectra, eng.full_size) == (4, 3, 96) and np.array_equal(eng.starts, 16 * np.arange(4))
    elif plan == "n2048 split":
        assert eng.num_windows == 5 and 3 * 2 <= info["grid"]    # launch_split: few frames on many CUs are split by windows
    else:
        assert eng.num_windows == 5 and eng.pfb_taps == 0
    full, w = eng.full_size, eng.hm_width
    raw, ref = in_format(stream((frames - 1) * stride + full, 77 + n), fmt)
    iq = Guarded.input(torch, raw, misalign={0: 8, 1: 2, 2: 2, 3: 4}[fmt], name="iq")
    cap = frames + 2
    out = Guarded.output(torch, cap * n * 4, name="out").own(0, frames * n * 4)
    eng.curscan_dev(iq.ptr, fmt, frames, out.ptr, frame_stride=stride)
    eng.synchronize()
    iq.check()
    out.check()
    lin = out.read(F32, frames * n).reshape(frames, n)
    picks = sorted({0, frames // 2, frames - 1})
    want = {f: oracle(ref[f * stride:f * stride + full]) for f in picks}
    for f in picks:
        (assert_psd if fold == "PSD" else assert_lin)(lin[f], want[f], what="%s fmt %d frame %d" % (plan, fmt, f))
    db = Guarded.output(torch, cap * n * 4, name="cur_db").own(0, frames * n * 4)
    hm = Guarded.output(torch, cap * w * 4, name="hm_rows").own(0, frames * w * 4)
    eng.frames_dev(iq.ptr, fmt, frames, cur_db=db.ptr, hm_rows=hm.ptr, frame_stride=stride)
    eng.synchronize()
    for gbuf in (iq, db, hm):
        gbuf.check()
    rows = db.read(F32, frames * n).reshape(frames, n)
    for f in picks:
        tag = "%s fmt %d dB frame %d" % (plan, fmt, f)
        if fold == "PSD":       # (a density: held to assert_psd's tolerance after undoing the dB step)
            assert_psd(10.0 ** ((rows[f].astype(np.float64) + eng.gain) / 10), want[f], what=tag)
        else:
            assert_db(rows[f], orc.log_no_gain(np.asarray(want[f], dtype=np.float64), eng.gain), what=tag)
    _same(hm.read(F32, frames * w).reshape(frames, w), sm.scan_rows(rows, None, w, 0), "%s fmt %d waterfall rows" % (plan, fmt))
    st = eng.state()
    _same(st["Fft.Cur"].astype(F32), rows[-1], "%s fmt %d Cur" % (plan, fmt))
    last = min(frames, 128)
    _same(sm.ring_rows(st["fftHM"].astype(F32), st["hm_index"], last), sm.scan_rows(rows[-last:], None, w, 0), "%s fmt %d ring" % (plan, fmt))
    _note("spectrum buffers")
    eng.close()


# ------------------------------------------------------------------------------------------------ coverage
# kernel of ksa_kernels.hpp -> the tests of this file that launch it and check what it wrote.  Fourteen of the fifteen
# untemplated kernels: combine_parts_kernel has a `recipe` in the catalogue, not a `covered_by` record, so it is not in this
# table; test_spectrum_stage_buffers["n2048 split"] launches it all the same (its dB rows are held against the oracle).
COVERS = {
    "accumulate_partial_kernel": ("test_accumulate_counts_around_the_launch_plan", "test_accumulate_split_runs"),
    "accumulate_reduce_kernel": ("test_accumulate_counts_around_the_launch_plan", "test_accumulate_split_runs",
                                 "test_accumulate_where_max_chunks_sets_the_chunk_count"),
    "commit_kernel": ("test_accumulate_flags_toggled_between_batches", "test_accumulate_split_runs"),
    "merge_gathered_kernel": ("test_merge_gathered_blocks_of_its_own_choosing",),
    "db_rows_kernel": ("test_frame_spectrum_rows_state_and_ring",),
    "rowmax_batch": ("test_spectrum_stage_buffers",),
    "scan_stitch_kernel": ("test_stitch_of_injected_bands", "test_stitch_shards_equal_one_engine"),
    "rowmax_kernel": ("test_stitch_of_injected_bands", "test_view_of_the_scan_state"),
    "rowmax_rows_kernel": ("test_stitch_of_injected_bands", "test_stitch_with_cells_wider_than_a_wave"),
    "rowmax_rows_range_kernel": ("test_stitch_shards_equal_one_engine",),
    "scan_merge_rows_kernel": ("test_stitch_shards_equal_one_engine",),
    "levels_kernel": ("test_levels_of_injected_zero_span_state", "test_levels_of_injected_scan_state"),
    "highs_kernel": ("test_highs_of_injected_curves", "test_view_equals_the_separate_calls_and_the_model"),
    "fill_kernel": ("test_view_of_the_scan_state",),
}


def test_every_state_kernel_is_named_here():
    """Every `covered_by` kernel of the main library is named by a test of this file, the catalogue names that test, and the
    test exists.  Then the figures of the run (cases and the worst error over its bound) are printed."""
    main = {r["kernel"][len("ksa::"):]: r["covered_by"] for r in kc.RECORDS if r["lib"] == "libksa.so" and "covered_by" in r}
    assert set(main) == set(COVERS), set(main) ^ set(COVERS)
    for kernel, tests in COVERS.items():
        for t in tests:
            assert callable(globals().get(t)), t
            assert kc.G % ("state_sweep", t) in main[kernel], "%s: the catalogue does not name %s" % (kernel, t)
    for name in sorted(SEEN):
        print("state sweep: %-18s %6d cases%s" % (name, SEEN[name], "   worst error / bound %.3g" % WORST[name] if name in WORST else ""))
