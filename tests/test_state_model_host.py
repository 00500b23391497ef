"""tests/state_model.py on the CPU: the models agree with oracle/ksa_oracle.py where the oracle defines the result
(plot_highs, plotcompress, data_cumu, ScanState.run_pass), and each of them notices a planted error of the kind the GPU sweep
(tests/test_gpu_state_sweep.py) exists to catch."""
import numpy as np
import pytest

import ksa_oracle as orc
import state_model as sm

F32 = np.float32


def _curve(rng, n, lo=-90.0, hi=-10.0):
    return rng.uniform(lo, hi, n).astype(F32)


# ------------------------------------------------------------------------------------------------ highs
@pytest.mark.parametrize("cells,count,sep", [(64, 5, 3.5), (64, 64, 0.5), (1025, 7, 40.25), (3, 2, 1.5), (2, 1, 0.0), (4096, 63, 64.5),
                                             (512, 5, 700.5)])
def test_highs_equals_plot_highs_on_tie_free_curves(cells, count, sep):
    """Tie-free levels and a spacing away from a multiple of the cell width: what the reference pins (ksa.h on ksa_read_highs)."""
    rng = np.random.default_rng(cells * 131 + count)
    lv = rng.permutation(cells).astype(F32) * F32(0.25) - F32(70)        # distinct by construction
    if cells > 8:
        a, b = rng.choice(cells, 2, replace=False)
        lv[a], lv[b] = np.nan, np.inf                                    # one NaN (sorts last in both) above one +inf: still tie-free
    freqs = 88e6 + 2.4e6 * np.arange(cells) / cells                      # a uniform axis, cell width 2.4e6 / cells
    frac = sep * (freqs[1] - freqs[0]) / (freqs[-1] - freqs[0]) if cells > 1 else 0.0
    ref = orc.plot_highs(freqs, lv.astype(np.float64), frac, count)
    marks, lvl, found = sm.highs(lv, sep, count)
    assert found == len(ref) == len(marks)
    assert [int(round((f - freqs[0]) / (freqs[1] - freqs[0]))) for f, _ in ref] == marks
    assert np.array_equal([l for _, l in ref], lv[marks].astype(np.float64), equal_nan=True)
    assert np.array_equal(np.asarray(lvl, dtype=np.float64), lv[marks].astype(np.float64), equal_nan=True)
    if (cells, count) == (64, 64):
        assert found == 63                                               # the curve runs out: the lowest point is never visited
    if sep > cells:
        assert found == 1


def test_highs_rules_of_the_header():
    """The lowest point is never visited, ties go higher index first, both zeros are one level, NaN comes first."""
    assert sm.highs(np.array([5.0], F32), 0.0, 4) == ([], [], 0)                      # one cell: position 0 only
    assert sm.highs(np.array([1.0, 1.0], F32), 0.0, 4)[0] == [1]                       # index 0 is sorted position 0
    assert sm.highs(np.array([-1, 0.0, -0.0, -2, -0.0, 0.0], F32), 0.0, 4)[0] == [5, 4, 2, 1]
    assert sm.highs(np.array([0, np.nan, np.inf, np.nan, 3], F32), 0.0, 3)[0] == [3, 1, 2]
    assert sm.highs(np.array([0, 9, 8, 7, 6, 5], F32), 2.0, 5)[0] == [1, 3, 5]         # spacing of exactly min_sep is allowed
    assert sm.highs(np.array([0, 9, 8, 7, 6, 5], F32), 2.0 + 2.0 ** -40, 5)[0] == [1, 4]
    assert sm.highs(np.full(7, np.nan, F32), 1e9, 64)[0] == [6]                        # found < count
    # a planted error: a result that marked the lowest point too.  Only a curve with a still lower point behind it gives that
    # through the model, so the model tells the two apart
    lv = np.array([3, 2, 1], F32)
    visited_lowest = [0, 1, 2]
    assert sm.highs(lv, 0.0, 3)[0] == [0, 1] != visited_lowest and sm.highs(np.append(lv, F32(-np.inf)), 0.0, 3)[0] == visited_lowest


# ------------------------------------------------------------------------------------------------ levels
@pytest.mark.parametrize("n,cells", [(16, 1), (16, 16), (1500, 125), (1500, 375), (4096, 2), (16 * 129, 129)])
def test_levels_equal_plotcompress(n, cells):
    rng = np.random.default_rng(n + cells)
    state = np.array([_curve(rng, n) for _ in range(4)])
    adj = _curve(rng, n, -3, 3)
    for a in (None, adj):
        src = state if a is None else (state - a[None, :]).astype(F32)
        for mode in ("MAX", "AVG"):
            got = sm.levels(state, a, cells, mode)
            want = np.array([orc.plotcompress(src[c].astype(np.float64), cells, mode) for c in range(4)])
            if mode == "MAX":
                assert np.array_equal(got.astype(np.float64), want)
            else:       # np.average's pairwise float64 sum against the exact one: the float32 result may sit one ulp apart
                assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(F32)))
        mn = sm.levels(state, a, cells, "MIN")
        assert np.array_equal(mn, src.reshape(4, cells, n // cells).min(axis=2))


def test_levels_special_values_and_planted_cell_shift():
    v = np.array([[1, np.nan, 3, 4, np.inf, -np.inf, 7, 8, np.inf, 1, -0.0, 0.0, -np.inf, -np.inf, 2, -5]], F32)
    for mode in ("AVG", "MAX", "MIN"):
        got = sm.levels(v, None, 8, mode)[0]
        assert np.isnan(got[0]) and got[1] == {"AVG": 3.5, "MAX": 4, "MIN": 3}[mode]
    assert np.isnan(sm.levels(v, None, 8, "AVG")[0][2])                  # +inf and -inf in one cell
    assert sm.levels(v, None, 8, "MAX")[0][2] == np.inf and sm.levels(v, None, 8, "MIN")[0][2] == -np.inf
    assert sm.levels(v, None, 8, "AVG")[0][4] == np.inf and sm.levels(v, None, 8, "AVG")[0][6] == -np.inf
    # a planted error: cells that start one bin late
    rng = np.random.default_rng(5)
    s = _curve(rng, 64)[None, :]
    for mode in ("AVG", "MAX", "MIN"):
        assert not np.array_equal(sm.levels(s, None, 8, mode), sm.levels(np.roll(s, -1, axis=1), None, 8, mode))


# ------------------------------------------------------------------------------------------------ rows and rings
def test_ring_rows_view_and_db_rows():
    ring = np.arange(128 * 4, dtype=F32).reshape(128, 4)
    assert np.array_equal(sm.ring_rows(ring, 1, 3)[:, 0] // 4, [126, 127, 0])
    assert sm.ring_rows(ring, 0, 0).shape == (0, 4) and np.array_equal(sm.ring_rows(ring, 5, 128)[0], ring[5])
    rng = np.random.default_rng(3)
    state = np.array([_curve(rng, 64) for _ in range(4)])
    lv, marks, lvl, found, rows, idx = sm.view(state, None, ring, 127, 16, "MAX", 3, 2.5, 5, 2)
    assert np.array_equal(lv, sm.levels(state, None, 16, "MAX")) and (marks, lvl, found) == sm.highs(lv[3], 2.5, 5)
    assert np.array_equal(rows, ring[[125, 126]]) and idx == 127
    mag = np.array([0.0, 1e-3, np.nan, np.inf, 2.0, 1e-40, 4.0, 8.0])
    adj = np.linspace(-1, 1, 8)
    db, row = sm.db_rows(mag, 19.1, adj, 4)
    st = orc.ZeroSpanState(8, 4, 19.1, adj=adj)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = st.push(mag.copy())
    assert np.array_equal(db, want, equal_nan=True) and np.array_equal(row, st.hm[0], equal_nan=True)
    assert db[0] == -np.inf and np.isnan(row[1]) and row[0] == db[1] - adj[1]
    # a planted error: a row stored one ring slot late
    assert not np.array_equal(sm.ring_rows(ring, 6, 4), sm.ring_rows(ring, 7, 4))


# ------------------------------------------------------------------------------------------------ accumulate
def _oracle_run(rows, state, flags):
    cur, mx, mn, av = state
    n = rows.shape[1]
    with np.errstate(invalid="ignore"):
        for pr in rows.astype(np.float64):
            cur = pr
            if flags[0]:
                mx = orc.data_cumu(orc.CUMU_MAX, mx, 0, n, pr, 0, n)
            if flags[1]:
                mn = orc.data_cumu(orc.CUMU_MIN, mn, 0, n, pr, 0, n)
            if flags[2]:
                av = orc.data_cumu(orc.CUMU_AVG, av, 0, n, pr, 0, n)
    return [cur, mx, mn, av]


def _acc_rows(rng, k, n):
    rows = _curve(rng, k * n).reshape(k, n)
    rows[0, 1] = -np.inf
    rows[k - 1, 2] = np.nan
    rows[k // 2, 3] = -np.inf
    return rows


@pytest.mark.parametrize("k", [1, 2, 64, 129, 300])
def test_accumulate_equals_data_cumu(k):
    rng = np.random.default_rng(k)
    n = 8
    rows = _acc_rows(rng, k, n)
    got, has = sm.accumulate(rows, 0, k, None, (0, 0, 0), (1, 1, 1))
    want = _oracle_run(rows, [None] * 4, (1, 1, 1))
    for g, w in zip(got, want):
        assert np.array_equal(g, w, equal_nan=True)
    assert has == (True, True, True)
    # a second committed batch on top, with Min switched off and then on again: Min is seeded by copy (K:133-134)
    rows2 = _acc_rows(rng, 5, n)
    got2, has2 = sm.accumulate(rows2, 0, 5, got, has, (1, 0, 1))
    want2 = _oracle_run(rows2, [w.copy() for w in want], (1, 0, 1))
    for g, w in zip(got2, want2):
        assert np.array_equal(g, w, equal_nan=True)
    first, has_f = sm.accumulate(rows, 0, k, None, (0, 0, 0), (1, 0, 1))
    assert has_f == (True, False, True) and np.all(first[2] == 0)
    late, _ = sm.accumulate(rows2, 0, 5, first, has_f, (1, 1, 1))
    assert np.array_equal(late[2], rows2.astype(np.float64).min(axis=0), equal_nan=True)


def test_accumulate_shards_add_up_and_a_missing_chunk_shows():
    """Two shards of one run (each with the other's frames absent) sum to the run's Avg; leaving 64 frames out does not."""
    rng = np.random.default_rng(11)
    k, n = 200, 4
    rows = _curve(rng, k * n).reshape(k, n)
    whole, _ = sm.accumulate(rows, 0, k, None, (0, 0, 0), (1, 1, 1))
    tail, _ = sm.accumulate(rows[120:], 120, k, None, (0, 0, 0), (1, 1, 1))
    z = rows.copy()
    z[120:] = 0
    head, _ = sm.accumulate(z, 0, k, None, (0, 0, 0), (1, 1, 1))
    assert np.allclose(head[3] + tail[3], whole[3], rtol=1e-13, atol=0)
    short = np.delete(rows, slice(128, 192), axis=0)
    wrong, _ = sm.accumulate(short, 0, k - 64, None, (0, 0, 0), (1, 1, 1))
    assert not np.allclose(wrong[3], whole[3], rtol=1e-6) or not np.array_equal(wrong[1], whole[1])
    with pytest.raises(AssertionError):
        sm.accumulate(rows[:10], 0, k, None, (0, 0, 0), (1, 1, 1))      # Cur is the run's last frame


# ------------------------------------------------------------------------------------------------ merge
def test_merge_gathered_rank_order_ring_and_planted_rank():
    rng = np.random.default_rng(2)
    n, w, world, fpr, idx0 = 8, 4, 3, 50, 127
    blocks = rng.normal(size=(world, 4 * n + 128 * w)).astype(F32) * F32(1e3)
    blocks[1, 3] = np.nan
    ring0 = np.full((128, w), 7, F32)
    part, ring = sm.merge_gathered(blocks, world, fpr, idx0, w, ring0)
    assert np.isnan(part[0, 3]) and part[1, 0] == blocks[:, n].max()
    s = blocks[:, 3 * n:4 * n]
    assert np.array_equal(part[3], ((s[0] + s[1]).astype(F32) + s[2]).astype(F32))
    # 150 frames from slot 127 on: slots 127, 0..20 were written twice, the newer one by rank 2 (frames 128..149)
    rings = blocks[:, 4 * n:].reshape(world, 128, w)
    assert np.array_equal(ring[127], rings[2][127]) and np.array_equal(ring[20], rings[2][20])
    assert np.array_equal(ring[21], rings[0][21]) and np.array_equal(ring[48], rings[0][48]) and np.array_equal(ring[49], rings[1][49])
    # 10 frames only: the other rows keep the engine's
    _, small = sm.merge_gathered(blocks, 2, 5, 3, w, ring0)
    assert np.all(small[:3] == 7) and np.all(small[13:] == 7) and np.array_equal(small[8], rings[1][8])
    # a planted error: every block taken from the rank in front (the gathered blocks rotated by one rank) through the same model
    _, wrong = sm.merge_gathered(np.roll(blocks, 1, axis=0), world, fpr, idx0, w, ring0)
    assert np.array_equal(wrong[49], rings[0][49]) and not np.array_equal(wrong[49], ring[49])
    assert not any(np.array_equal(wrong[s], ring[s]) for s in range(128))
    assert np.array_equal(sm.commit_fresh(part)[2], -part[2])


# ------------------------------------------------------------------------------------------------ stitch
def _identity_db(monkeypatch):
    """ScanState.run_pass fed dB bands: its clip and log steps pass the values through."""
    monkeypatch.setattr(orc, "clip2minamp", lambda vals, min_amp: vals)
    monkeypatch.setattr(orc, "log_no_gain", lambda vals, gain, inf_to=None: np.array(vals, dtype=np.float64))


@pytest.mark.parametrize("q", [1.0, 0.75, 0.5, 0.25])
@pytest.mark.parametrize("base_is_raw", [False, True])
def test_stitch_equals_scan_state_run_pass(monkeypatch, q, base_is_raw):
    """Integer-valued bands keep every float32 step exact, so the float32 model and the float64 oracle must agree exactly."""
    n, groups, passes = 16, 5, 3
    ref = orc.ScanState(n, 0.0, float(groups * n), float(n), 0.0, 1.0, 8, scan_non_overlap=q, base_is_raw=base_is_raw)
    _identity_db(monkeypatch)
    total, hop, nsteps = ref.total, int(n * q), len(ref.centers)
    rng = np.random.default_rng(int(q * 100) + base_is_raw)
    state0 = rng.integers(-32, 32, size=(4, total)).astype(F32)
    ref.cur, ref.max, ref.min, ref.avg = (state0[c].astype(np.float64) for c in range(4))
    adj = rng.integers(-4, 4, size=total).astype(F32)
    ref.adj = adj.astype(np.float64)
    bands = rng.integers(-64, 64, size=(passes, nsteps, n)).astype(F32)
    for p in range(passes):
        ref.run_pass([bands[p, i].astype(np.float64) for i in range(nsteps)])
    state, avg_rows = sm.stitch(bands, n, hop, total, state0, True, base_is_raw)
    for c, want in enumerate((ref.cur, ref.max, ref.min, ref.avg)):
        assert np.array_equal(state[c].astype(np.float64), want), "curve %d" % c
    ring = sm.scan_rows(avg_rows, adj, 8, 0, ring=np.zeros((128, 8), F32))
    assert np.array_equal(ring[:passes].astype(np.float64), ref.hm[:passes])
    # a planted error: the second pass skipped
    skipped, _ = sm.stitch(bands[[0, 2]], n, hop, total, state0, True, base_is_raw)
    assert not np.array_equal(skipped[3], state[3])
    # on top of an existing state = one call over all the passes
    s1, r1 = sm.stitch(bands[:1], n, hop, total, state0, True, base_is_raw)
    s2, r2 = sm.stitch(bands[1:], n, hop, total, s1, False, base_is_raw)
    assert np.array_equal(s2, state) and np.array_equal(np.concatenate([r1, r2]), avg_rows)


def test_stitch_keeps_uncovered_elements_and_partial_rows_merge():
    n, hop, total = 16, 4, 96
    rng = np.random.default_rng(9)
    state0 = rng.normal(size=(4, total)).astype(F32)
    bands = rng.normal(size=(2, 10, n)).astype(F32)             # bands 0..9 reach element 9*4 + 16 = 52
    bands[1, 3, 5] = np.nan
    state, avg_rows = sm.stitch(bands, n, hop, total, state0, True, False)
    assert np.array_equal(state[:, 52:], state0[:, 52:]) and not np.array_equal(state[:, :52], state0[:, :52])
    assert np.isnan(state[0, 17]) and np.isnan(state[1, 17]) and np.isnan(avg_rows[1, 17]) and not np.isnan(avg_rows[0]).any()
    adj = rng.normal(size=total).astype(F32)
    full = sm.scan_rows(avg_rows, adj, 6, 0)
    cuts = [0, 20, 20, 50, 96]                                   # one shard owns nothing
    parts = [sm.scan_rows(avg_rows, adj, 6, 0, e_lo=a, e_hi=b) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.all(parts[1] == -np.inf) and np.isneginf(parts[0][0, 2])
    assert np.array_equal(sm.merge_rows(parts), full, equal_nan=True) and np.isnan(full[1, 1])


# ------------------------------------------------------------------------------------------------ the launch plan mirror
def test_chunk_plan_is_the_source_text():
    import os

    import large_model as lm
    for path, lines in sm.CHUNK_RULE_SOURCE.items():
        with open(os.path.join(lm.PKG_DIR, path)) as f:
            text = f.read()
        for line in lines:
            assert line in text, "%s no longer holds `%s`: restate the rule in state_model.chunk_plan" % (path, line)
    assert lm.source_constant("csrc/ksa_kernels.hpp", "HM_ROWS") == sm.HM_ROWS
    assert lm.source_constant("csrc/ksa_kernels.hpp", "HIGHS_MAX") == 64 and lm.source_constant("csrc/ksa_kernels.hpp", "AHEAD") == 32
    # the counts of the GPU sweep sit where the plan changes: one chunk up to 127 frames, two from 128; 16 chunks (one per
    # reduce group) up to 1087, 17 (two per group) at 1088; 127 or 128 chunks of 64 or 65 frames around 8192
    assert [sm.chunk_plan(k, 16) for k in (1, 127, 128, 129)] == [(1, 1, 1), (127, 1, 1), (64, 2, 1), (65, 2, 1)]
    assert [sm.chunk_plan(k, 16) for k in (1087, 1088, 1089)] == [(68, 16, 1), (64, 17, 2), (65, 17, 2)]
    assert [sm.chunk_plan(k, 16) for k in (8191, 8192, 8193)] == [(65, 127, 8), (64, 128, 8), (65, 127, 8)]
    assert sm.chunk_plan(5505, 65536) == (65, 85, 6)         # max_chunks (85 at 65536 bins), not nframes / 64 = 86, sets the count
