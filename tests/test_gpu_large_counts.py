"""The paths of seven companion libraries that only large counts reach, against their models.

The sibling files pin every library to its numpy model at small sizes.  The libraries change code path once a count crosses a
threshold, and these tests cross each one: a workgroup's second and third trip round the tile loop (corr, resamp), more than
256 tiles in the one-workgroup stitch and in the state scan (pulse), per-tile memory that has to grow (pulse), a serial stretch
per thread in the one-workgroup scan (track), a second launch with advanced base pointers (detect, mask), and host rows that
cross in several pieces through one staging buffer (detect, mask, density).

Every test asserts that it crossed its threshold, from kernel_info() or from the constants that tests/test_large_model_host.py
pins to the source text, and that its expected result is not trivial.  The models are too slow at these counts, so the expected
results come out of tests/large_model.py: small model runs on a pool, gathered; that gathering is proved against the full
models on the CPU.  Every comparison is np.array_equal or the models' own equality: no tolerance exists here.

The tensors a test allocates stay below 300 MiB; an object's own work buffers, sized by the max_in the count dictates, come on
top of that (173 MB for the correlator at (7, 3))."""
import importlib

import numpy as np
import pytest

import density_model as ddm
import detect_model as dm
import large_model as lm
import mask_model as mm
import pulse_model as pm
import resamp_model as rm
import track_model as tm
import test_gpu_pulse as tp
import test_gpu_resamp as tr
import test_gpu_track as tt
from conftest import load_pkg

pytestmark = pytest.mark.gpu

CONST = lm.EXPECTED_CONSTANTS                    # pinned to the source text in test_large_model_host.py
THRESHOLD = 10.0                                 # detect: dB above the floor, as in test_gpu_detect
ROW_BASE = 2 ** 33


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def module(name):
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd." + name)


def events_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and all(np.array_equal(a[k], b[k]) for k in a.dtype.names)


def gathered(torch, pool, idx):
    """pool[idx] in device memory, gathered there: float32 [len(idx)][row length]."""
    flat = np.ascontiguousarray(pool).view(np.float32).reshape(len(pool), -1)
    return torch.from_numpy(flat).cuda()[torch.from_numpy(np.asarray(idx, dtype=np.int64)).cuda()].contiguous()


# ------------------------------------------------------------------------------------------ 1. corr: more tiles than the grid
@pytest.mark.parametrize("shape", [(7, 3), (64, 1)], ids=str)
def test_corr_workgroups_walk_two_and_three_tiles(torch_cuda, shape):
    """The grid is capped at 16 workgroups per compute unit; 16 CUs + 3 blocks of two tiles each make every workgroup walk two
    tiles and six of them three, through the barrier before the next load_span, with w / tiles leaving a remainder."""
    torch, X = torch_cuda, module("corr")
    K, Q = shape
    G, thr = 5, 0.5
    W = 256 * (4 if Q > 2 else 8)
    block_len = W + 150 + K - 1
    nl = block_len - K + 1
    cap = CONST["corr.WG_PER_CU"] * torch.cuda.get_device_properties(0).multi_processor_count
    nblocks = cap + 3
    c, pool = lm.corr_pool(shape, 32, block_len, 21)
    pool_want = lm.corr_pool_model(pool, c, thr, G)
    idx = lm.draw(np.random.default_rng(K), np.arange(32), nblocks)
    want, want_total = lm.corr_expand(pool_want, idx)
    assert len(np.unique(idx)) == 32 and nblocks < want_total == len(want) <= 1 << 20
    assert (pool_want["counts"] == 0).any() and (want["metric"] == 1).sum() >= nblocks // 2, "the planted copies must be found"

    x = gathered(torch, pool, idx)
    assert x.shape == (nblocks, 2 * block_len) and x.data_ptr() % 16 == 0
    cr = X.Correlator(c, threshold=thr, guard=G, capacity=1 << 20, max_in=nblocks * block_len)
    assert cr.kernel_info()["tile_out"] == W and -(-nl // W) == 2
    stride = nl + 1
    metric = torch.full((nblocks * Q, stride), -7.0, dtype=torch.float32, device="cuda")
    corr = torch.full((nblocks * Q, stride, 2), -7.0, dtype=torch.float32, device="cuda")
    assert cr.blocks_dev(x, nblocks, block_len, metric=metric, corr=corr, out_stride=stride) == nl
    ev, total = cr.events()
    grid = cr.kernel_info()["grid"]
    print("large counts: corr %s grid %d, tiles %d, blocks %d, events %d" % (shape, grid, 2 * nblocks, nblocks, total))
    assert grid == cap and grid < 2 * nblocks and 2 * nblocks - 2 * grid == 6, "every workgroup walks two tiles, six walk three"
    assert total == want_total and events_equal(ev, want)
    # dense values: the first block, the last, the block whose tiles open the second trip, the one before it, and the block
    # whose tiles open the third trip
    sel = [0, cap // 2 - 1, cap // 2, cap, nblocks - 1]
    at = torch.tensor(sel, device="cuda")
    rho = metric.view(nblocks, Q, stride)[at].cpu().numpy()
    r = corr.view(nblocks, Q, stride, 2)[at].cpu().numpy()
    assert np.all(rho[:, :, nl:] == -7.0) and np.all(r[:, :, nl:] == -7.0), "nothing is written past the lags of a block"
    assert np.array_equal(rho[:, :, :nl], pool_want["rho"][idx[sel]])
    assert np.array_equal(np.ascontiguousarray(r[:, :, :nl]).view(np.complex64)[..., 0], pool_want["r"][idx[sel]])
    assert cr.state()["samples_in"] == 0
    cr.close()


# ------------------------------------------------------------------------------------------ 2. resamp: more tiles than GRID_MAX
@pytest.mark.parametrize("distinct", [False, True], ids=["same", "distinct"])
@pytest.mark.parametrize("shape,typ,kind", [((3, 2, 4), "f32", "int"), ((2, 3, 5), "c64", "pow2")], ids=str)
def test_resamp_more_tiles_than_the_grid(torch_cuda, shape, typ, kind, distinct):
    """2^20 + 1027 blocks of one tile each: the first 1027 workgroups walk a second tile.  Once every block reads the same
    samples (block_stride 0), so every row of the output is the model's one block; and once the blocks are drawn from a pool of
    64 different ones and lie end to end, so that a workgroup's second tile holds other samples than its first: a span that
    the next tile's loads overwrite too early, or a block read from the wrong place, shows only there."""
    torch, X = torch_cuda, module("resamp")
    L, M, P = shape
    rng = np.random.default_rng(L * 7 + M * 13 + P)
    taps, num, den = rm.exact_taps(rng, L * P, kind)
    J = 3
    bl = next(n for n in range(1, 64) if rm.block_out_count(n, L, M, P) >= J)
    assert rm.block_out_count(bl, L, M, P) == J and rm.block_out_count(bl - 1, L, M, P) < J
    nblocks = CONST["resamp.GRID_MAX"] + 1027
    pool = np.stack([rm.exact_samples(rng, bl, typ == "c64") for _ in range(64 if distinct else 1)])
    pool_want = np.stack([rm.exact_blocks(x, num, den, L, M, [0], bl)[0] for x in pool])
    assert pool_want.shape == (len(pool), J) and np.count_nonzero(pool_want[0]) >= 2
    assert len(np.unique(pool_want, axis=0)) == len(pool)
    rs = X.Resampler(L, M, taps, type=typ, max_in=nblocks * bl)
    assert rs.block_out_count(bl) == J and rs.kernel_info()["tile_out"] >= J
    per = 2 if typ == "c64" else 1
    out = torch.full((nblocks * (J + 1) * per,), -7.0, dtype=torch.float32, device="cuda")
    if distinct:
        idx = lm.draw(np.random.default_rng(bl), np.arange(len(pool)), nblocks)
        x = gathered(torch, pool, idx)
        assert x.shape == (nblocks, bl * per) and x.data_ptr() % 16 == 0
        want = pool_want[idx]
        assert rs.blocks_dev(x, nblocks, bl, block_stride=bl, out=out, out_stride=J + 1) == J
    else:
        keep, ptr = tr.to_dev(torch, pool[0])
        want = np.broadcast_to(pool_want[0], (nblocks, J))
        assert rs.blocks_dev(ptr, nblocks, bl, block_stride=0, out=out, out_stride=J + 1) == J
    rs.synchronize()
    grid = rs.kernel_info()["grid"]
    print("large counts: resamp %s %s %s blocks, grid %d, tiles %d" % (shape, typ, "distinct" if distinct else "the same", grid, nblocks))
    assert grid == CONST["resamp.GRID_MAX"] < nblocks
    full = tr.fetch(torch, out, nblocks * (J + 1), rs.dtype).reshape(nblocks, J + 1)
    assert np.array_equal(full[:, :J], want)
    fill = np.complex64(-7 - 7j) if typ == "c64" else np.float32(-7)
    assert np.all(full[:, J] == fill), "the padding column keeps its fill value"
    rs.close()


# ------------------------------------------------------------------------------------------ 3. pulse: 259 tiles in one stream call
PULSE_T = CONST["pulse.TILE"]
PULSE_N = 258 * PULSE_T + 5
PULSE_W, PULSE_ON, PULSE_OFF = 16, 0.06, 0.03
PLANTED = {"early": (PULSE_T + 1800, 2 * PULSE_T + 400),                   # a cut inside it carries an open run into 257 tiles
           "through": (100 * PULSE_T - 50, 104 * PULSE_T + 50),            # tiles 100 .. 103 active throughout
           "exact": (129 * PULSE_T - 10, 129 * PULSE_T + 10),              # a run of exactly min_len over tiles 128 | 129
           "long": (255 * PULSE_T + 700, 257 * PULSE_T + 300),             # from tile 255 into tile 257
           "last": (PULSE_N - 500, PULSE_N)}                               # ends on the stream's last sample


def pulse_stream(fmt):
    """(raw samples, min_len): bursty_s16 with the planted stretches of PLANTED, each strong and constant inside a margin of
    40 zero samples, so that the run it makes is its own; min_len is the length of the run the `exact` stretch makes."""
    iq = tp.bursty_s16(np.random.default_rng(259), PULSE_N)
    for a, b in PLANTED.values():
        iq[max(a - 40, 0):min(b + 40, PULSE_N)] = 0
        iq[a:b] = (12000, -9000)
    raw = iq if fmt == "s16" else ((iq[:, 0] + 1j * iq[:, 1]) / 32768.0 * 1.7).astype(np.complex64)
    a, b = PLANTED["exact"]
    alone = pm.detect(raw[a - 40:b + 40], PULSE_W, PULSE_ON, PULSE_OFF, 1, fmt)[1]
    assert len(alone) == 1 and alone[0]["flags"] == 0 and 8 <= alone[0]["len"] <= 60
    return raw, int(alone[0]["len"])


@pytest.mark.parametrize("fmt", ["c64", "s16"])
def test_pulse_stream_of_259_tiles(torch_cuda, fmt):
    """NT = 259 > 256: stitch_kernel gives every thread a stretch of C = 2 tiles (129 full stretches, one of a single tile, 126
    empty ones), state_kernel takes a second iteration with its carry.  Then the same samples in two calls, cut inside a run."""
    torch, X = torch_cuda, module("pulse")
    T, n, W = PULSE_T, PULSE_N, PULSE_W
    raw, min_len = pulse_stream(fmt)
    wS, wev, act = pm.detect(raw, W, PULSE_ON, PULSE_OFF, min_len, fmt)
    start, end = wev["start"], wev["start"] + wev["len"]
    assert len(wev) > 300
    assert np.any((start // T == 255) & ((end - 1) // T == 257)), "a run from tile 255 into tile 257"
    assert np.any((start < 100 * T) & (end > 104 * T)), "tiles 100 .. 103 active throughout"
    assert np.any((wev["len"] == min_len) & (start < 129 * T) & (end > 129 * T)), "a run of exactly min_len over tiles 128 | 129"
    assert wev[-1]["flags"] == pm.FLAG_OPEN_END and end[-1] == n and np.all(wev["flags"][:-1] == 0)
    cut_late, cut_early = 256 * T + 100, 2 * T - 37
    for cut in (cut_late, cut_early):
        assert np.any((start < cut) & (end > cut)) and act[cut - 1] and act[cut], "the cut lies inside a run"
    assert -(-cut_late // T) == 257 and -(-(n - cut_early) // T) == 257

    det = X.PulseDetector(W=W, on_power=PULSE_ON, off_power=PULSE_OFF, min_len=min_len, capacity=4096, max_in=n, fmt=fmt)
    assert det.kernel_info()["tile"] == T and det.thresholds() == pm.thresholds(PULSE_ON, PULSE_OFF, W)
    keep, ptr = tp.to_dev(torch, raw)
    per = tp.sample_bytes(raw)
    closed = wev[:-1]
    for pieces in ([n], [cut_late, n - cut_late], [cut_early, n - cut_early]):
        det.reset()
        env = torch.full((n + 3,), -7, dtype=torch.int64, device="cuda")
        at, grids = 0, []
        for p in pieces:
            det.process_dev(ptr + per * at, p, env=env.data_ptr() + 8 * at)
            at += p
            grids.append(det.kernel_info()["grid"])
            if at < n:                                               # the first call leaves its run open
                run = wev[(start < at) & (end > at)][0]
                assert det.state() == {"samples_in": at, "open": True, "open_start": int(run["start"])}
        assert grids == [-(-p // T) for p in pieces] and max(grids) > CONST["pulse.THREADS"]
        print("large counts: pulse stream %s pieces %s grids %s, pulses %d, min_len %d" % (fmt, pieces, grids, len(wev), min_len))
        ev, total, active = det.events()
        assert total == len(closed) and active == int(closed["len"].sum()) and tp.events_equal(ev, closed)
        assert det.state() == {"samples_in": n, "open": True, "open_start": int(start[-1])}
        det.flush()
        ev, total, active = det.events()
        assert total == len(wev) and active == int(wev["len"].sum()) and tp.events_equal(ev, wev)
        assert det.state() == {"samples_in": n, "open": False, "open_start": -1}
        S = env.cpu().numpy()
        assert np.all(S[n:] == -7) and np.array_equal(S[:n], wS)
    det.close()


# ------------------------------------------------------------------------------------------ 4. pulse: 700 short blocks
def test_pulse_700_short_blocks_grow_the_tile_memory(torch_cuda):
    """700 blocks of one tile each on an object made for 52 tiles: ensure_tiles re-allocates, stitch_kernel takes C = 3 tiles
    per thread, and every stretch straddles block ends, where `final` closes the open run."""
    torch, X = torch_cuda, module("pulse")
    nblocks, blen, stride, W, on, off = 700, 150, 100, 7, 0.05, 0.02
    max_in = nblocks * blen
    assert nblocks > -(-max_in // PULSE_T) + 1 == 53 and -(-nblocks // CONST["pulse.THREADS"]) == 3
    rng = np.random.default_rng(700)
    raw = tp.bursty_s16(rng, (nblocks - 1) * stride + blen, period=60)
    parts = [pm.detect(raw[b * stride:b * stride + blen], W, on, off, 1, "s16", block=b, flushed=True) for b in range(nblocks)]
    want = np.concatenate([p[1] for p in parts])
    wS = np.stack([p[0] for p in parts])
    open_blocks = len(set(want["block"][want["flags"] == pm.FLAG_OPEN_END]))
    assert open_blocks >= 50 and len(want) > 2 * nblocks
    det = X.PulseDetector(W=W, on_power=on, off_power=off, min_len=1, capacity=1 << 14, max_in=max_in, fmt="s16")
    keep, ptr = tp.to_dev(torch, raw)
    env = torch.full((nblocks, blen + 3), -7, dtype=torch.int64, device="cuda")
    det.blocks_dev(ptr, nblocks, blen, block_stride=stride, env=env, out_stride=blen + 3)
    ev, total, active = det.events()
    grid = det.kernel_info()["grid"]
    print("large counts: pulse blocks grid %d (made for 53 tiles), pulses %d, blocks with an open end %d" % (grid, total, open_blocks))
    assert grid == nblocks
    assert total == len(want) and active == int(want["len"].sum()) and tp.events_equal(ev, want)
    S = env.cpu().numpy()
    assert np.all(S[:, blen:] == -7) and np.array_equal(S[:, :blen], wS)
    assert det.state() == {"samples_in": 0, "open": False, "open_start": -1}
    # the object survives the re-allocation: an ordinary stream call still matches its model
    det.clear_events()
    raw2 = tp.bursty_s16(rng, 3 * PULSE_T + 5)
    wev = tp.check_against_model(tp.run_stream(torch, det, raw2), raw2, W, on, off, fmt="s16")
    assert len(wev) > 5
    det.close()


# ------------------------------------------------------------------------------------------ 5. track: 327 685 spans
def test_track_327685_spans_take_two_counts_per_scan_thread(torch_cuda):
    """Five copies of the 65 537-span list: 1281 workgroups of mark feed the 1024 threads of scan_kernel, per = 2, thread 640
    holds one count, the threads behind it none."""
    X = module("track")
    n0, k, row_gap, slop = 65537, 5, 1, 1
    s = tt.random_list()[:n0]
    spans, row_end = lm.track_copies(s, k, row_gap)
    n = len(spans)
    blocks = -(-n // CONST["track.THREADS"])
    assert n == 327685 and blocks == 1281 and -(-blocks // CONST["track.SCAN_THREADS"]) == 2
    assert row_end > int(spans["row"][-1]) + row_gap + 1
    one_end = int(s["row"][-1]) + 1 + row_gap + 2

    def link(capacity, **kw):
        trk = X.EmissionTracker(tt.NBINS, row_gap=row_gap, bin_slop=slop, capacity=capacity, max_spans=n, **kw)
        try:
            assert trk.kernel_info()["grid"] == blocks
            labels = trk.link(spans, row_end)
            return trk.tracks() + (labels,)
        finally:
            trk.close()

    one = tm.link(s, tt.NBINS, one_end, row_gap, slop, capacity=1 << 20)
    want = lm.track_expand(one, s, k, row_gap)
    assert want[1] == k * one[1] > 10000 and want[0]["nspans"].max() >= 12 and np.count_nonzero(want[0]["nspans"] == 1) >= 5
    tt.agree(link(want[1]), want)
    print("large counts: track spans %d, workgroups %d, counts per scan thread 2, tracks %d" % (n, blocks, want[1]))
    half = want[1] // 2                                              # the first half of the records, every label
    cut = lm.track_expand(one, s, k, row_gap, capacity=half)
    assert len(cut[0]) == half and tm.same_records(cut[0], want[0][:half]) and np.array_equal(cut[3], want[3])
    tt.agree(link(half), cut)
    one = tm.link(s, tt.NBINS, one_end, row_gap, slop, min_rows=3, capacity=1 << 20)      # filtered roots in the scan as well
    want3 = lm.track_expand(one, s, k, row_gap)
    assert 0 < want3[1] < want3[2] == want[2] and (want3[3] == -1).any()
    tt.agree(link(want3[1], min_rows=3), want3)


# ------------------------------------------------------------------------------------------ 6. detect: a second launch
def edge_rows(n, edge):
    """The first 3 rows, the 7 around `edge`, the last 3."""
    return np.concatenate([np.arange(3), np.arange(edge - 3, edge + 4), np.arange(n - 3, n)])


@pytest.mark.parametrize("mode", ["ca", "go"])
def test_detect_rows_beyond_one_launch(torch_cuda, mode):
    """2^20 + 300 rows in one call: launch_detect takes a second launch with rows, row_count and floor advanced, row_base moved
    on, the running total snapshot and the per-row scratch reused.  Once more from an unaligned base (the 4-byte form)."""
    torch, X = torch_cuda, module("detect")
    edge, nbins, train, guard = CONST["detect.MAX_LAUNCH_ROWS"], 16, 4, 1
    n = edge + 300
    pool, cand = lm.detect_pool(512, nbins)
    idx = lm.draw(np.random.default_rng(6), cand, n)
    pool_want = lm.detect_pool_model(pool, train, guard, THRESHOLD, mode)
    assert np.isnan(pool).any() and np.isinf(pool).any()
    rows = gathered(torch, pool, idx)

    def run(dev, nrows, vec, want_floor):
        compared = edge_rows(nrows, edge)
        want = lm.detect_expand(pool_want, idx[:nrows], ROW_BASE, 1 << 20, compared)
        assert 100000 < want["total"] == len(want["events"]) and (want["count"] == 0).sum() > nrows // 2
        count = torch.full((nrows,), -7, dtype=torch.int32, device="cuda")
        floor = torch.full((nrows, nbins), 123.0, dtype=torch.float32, device="cuda") if want_floor else None
        det = X.SignalDetector(nbins, train, guard, THRESHOLD, mode=mode, capacity=1 << 20)
        det.set_row_base(ROW_BASE)
        det.detect_rows_dev(dev, nrows, row_stride=nbins, row_count=count, floor=floor)
        hits, seen = det.hits()
        ev, total = det.emissions()
        assert det.kernel_info()["vec"] == vec
        det.close()
        assert seen == ROW_BASE + nrows and total == want["total"]
        assert dm.emissions_equal(ev, want["events"])
        assert np.any(ev["row"] < ROW_BASE + edge) and np.any(ev["row"] >= ROW_BASE + edge), "emissions on both sides of 2^20"
        assert np.array_equal(hits, want["hits"]) and hits.sum() > 0
        assert np.array_equal(count.cpu().numpy(), want["count"])
        if want_floor:
            got = floor[torch.from_numpy(compared).cuda()].cpu().numpy()
            assert dm.floors_equal(got, want["floor"]) and not np.any(got == 123.0)
        return total

    total = run(rows, n, 1, True)
    print("large counts: detect %s rows %d (one launch takes %d), emissions %d" % (mode, n, edge, total))
    if mode == "ca":
        n2 = edge + 5
        flat = torch.empty(1 + n2 * nbins, dtype=torch.float32, device="cuda")
        flat[1:] = rows[:n2].reshape(-1)
        assert flat[1:].data_ptr() % 16 == 4
        run(flat[1:], n2, 0, False)


# ------------------------------------------------------------------------------------------ 7. mask: a second launch
def test_mask_rows_beyond_one_launch(torch_cuda):
    torch, X = torch_cuda, module("mask")
    edge, nbins = CONST["mask.MAX_LAUNCH_ROWS"], 16
    n = edge + 300
    pool, up, lo = lm.mask_pool(512, nbins, True)
    idx = lm.draw(np.random.default_rng(7), np.arange(512), n)
    want = lm.mask_expand(lm.mask_pool_model(pool, up, lo, 1), idx, ROW_BASE)
    assert 100000 < want["total"] == len(want["events"]) < n // 2 and np.all(want["hits"].sum(axis=1) > 0)
    rows = gathered(torch, pool, idx)
    flag = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    m = X.SpectrumMask(nbins, up, lo, min_bins=1, capacity=1 << 20)
    m.set_row_base(ROW_BASE)
    m.check_rows_dev(rows, n, row_event=flag)
    hits, seen = m.hits()
    ev, total = m.events()
    m.close()
    print("large counts: mask rows %d (one launch takes %d), events %d" % (n, edge, total))
    assert seen == ROW_BASE + n and total == want["total"]
    assert mm.events_equal(ev, want["events"])
    assert np.any(ev["row"] < ROW_BASE + edge) and np.any(ev["row"] >= ROW_BASE + edge), "events on both sides of 2^20"
    assert np.array_equal(hits, want["hits"])
    assert np.array_equal(flag.cpu().numpy(), want["event"].astype(np.uint8))


# ------------------------------------------------------------------------------------------ 8. host rows in several pieces
def pieces_of(lib, nbins):
    """(rows per piece, rows of the test): two whole pieces and a short third."""
    piece = CONST[lib + ".STAGE_BYTES"] // (4 * nbins)
    return piece, 2 * piece + 37


def piece_rows(n, piece):
    return np.concatenate([np.arange(piece - 3, piece + 4), np.arange(2 * piece - 3, 2 * piece + 4), np.arange(n - 5, n)])


def test_detect_host_rows_cross_in_three_pieces(torch_cuda):
    torch, X = torch_cuda, module("detect")
    nbins, train, guard = 16384, 32, 2
    piece, n = pieces_of("detect", nbins)
    assert (piece, n) == (1024, 2085)
    pool, cand = lm.detect_pool(64, nbins, without_combs=True)
    idx = lm.draw(np.random.default_rng(8), cand, n)
    rows = pool[idx]
    assert 128 << 20 <= rows.nbytes <= 135 << 20
    host = X.SignalDetector(nbins, train, guard, THRESHOLD, capacity=1 << 16)
    host.detect_rows(rows)
    dev = X.SignalDetector(nbins, train, guard, THRESHOLD, capacity=1 << 16)
    up = torch.from_numpy(rows).cuda()
    dev.detect_rows_dev(up, n)
    got = {}
    for name, det in (("host", host), ("dev", dev)):
        got[name] = det.hits() + det.emissions()
        det.close()
    del up
    a, b = got["host"], got["dev"]
    print("large counts: detect host rows %d in pieces of %d, emissions %d" % (n, piece, a[3]))
    assert a[1] == b[1] == n and a[3] == b[3] and np.array_equal(a[0], b[0]) and a[2].tobytes() == b[2].tobytes()
    want = lm.detect_expand(lm.detect_pool_model(pool, train, guard, THRESHOLD, "ca"), idx, 0, 1 << 16)
    compared = piece_rows(n, piece)
    assert 1000 < want["total"] <= 1 << 16 and len(lm.rows_of(want["events"], compared)) > 10
    assert dm.emissions_equal(lm.rows_of(b[2], compared), lm.rows_of(want["events"], compared))
    assert b[3] == want["total"] and dm.emissions_equal(b[2], want["events"]) and np.array_equal(b[0], want["hits"])


def test_mask_host_rows_cross_in_three_pieces(torch_cuda):
    torch, X = torch_cuda, module("mask")
    nbins = 4096
    piece, n = pieces_of("mask", nbins)
    assert (piece, n) == (4096, 8229)
    pool, up_line, lo_line = lm.mask_pool(64, nbins, True)
    idx = lm.draw(np.random.default_rng(9), np.arange(64), n)
    rows = pool[idx]
    assert 128 << 20 <= rows.nbytes <= 135 << 20
    host = X.SpectrumMask(nbins, up_line, lo_line, capacity=1 << 16)
    host.check_rows(rows)
    dev = X.SpectrumMask(nbins, up_line, lo_line, capacity=1 << 16)
    up = torch.from_numpy(rows).cuda()
    dev.check_rows_dev(up, n)
    got = {}
    for name, m in (("host", host), ("dev", dev)):
        got[name] = m.hits() + m.events()
        m.close()
    del up
    a, b = got["host"], got["dev"]
    print("large counts: mask host rows %d in pieces of %d, events %d" % (n, piece, a[3]))
    assert a[1] == b[1] == n and a[3] == b[3] and np.array_equal(a[0], b[0]) and a[2].tobytes() == b[2].tobytes()
    want = lm.mask_expand(lm.mask_pool_model(pool, up_line, lo_line, 1), idx, 0, 1 << 16)
    compared = piece_rows(n, piece)
    assert 1000 < want["total"] <= 1 << 16 and len(lm.rows_of(want["events"], compared)) >= 3
    assert mm.events_equal(lm.rows_of(b[2], compared), lm.rows_of(want["events"], compared))
    assert b[3] == want["total"] and mm.events_equal(b[2], want["events"]) and np.array_equal(b[0], want["hits"])


def test_density_host_rows_cross_in_three_pieces(torch_cuda):
    torch, X = torch_cuda, module("density")
    nbins, levels, lo_db, hi_db = 4096, 256, -140.0, 0.0
    piece, n = pieces_of("density", nbins)
    assert (piece, n) == (4096, 8229)
    pool, _, _ = lm.mask_pool(64, nbins, True)                       # infinities and NaN among the values
    idx = lm.draw(np.random.default_rng(10), np.arange(64), n)
    rows = pool[idx]
    assert 128 << 20 <= rows.nbytes <= 135 << 20
    host = X.SpectrumDensity(nbins, levels=levels, lo_db=lo_db, hi_db=hi_db)
    host.add_rows(rows)
    dev = X.SpectrumDensity(nbins, levels=levels, lo_db=lo_db, hi_db=hi_db)
    up = torch.from_numpy(rows).cuda()
    dev.add_rows_dev(up, n)
    a, b = host.read(), dev.read()
    width = a[0].shape[1]
    host.close()
    dev.close()
    del up
    print("large counts: density host rows %d in pieces of %d, width %d" % (n, piece, width))
    assert a[1] == b[1] == n and np.array_equal(a[0], b[0]) and a[0].dtype == np.int64
    want = ddm.histogram(rows, width, levels, lo_db, hi_db)
    assert np.array_equal(b[0], want) and want.sum() == n * nbins and want[levels].sum() > 0 and np.count_nonzero(want) > 1000
