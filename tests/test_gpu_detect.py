"""The CFAR signal detector on the GPU against its integer model (tests/detect_model.py).  Every comparison is exact:
np.array_equal on the hits, the per-row counts and every field of the emission records (peak_db and floor_db by their bits), the
floor line by its NaN positions and its bits elsewhere.  Shapes are the smallest at which the row pass takes each of its paths:
several rows per wave (16, 18, 64 bins), several waves per row, one and several tiles per row (1024, 4096, 16384 bins), a row
that is no multiple of four (the 4-byte form), one and several workgroups of the scan, and, at 16 and 18 bins, more passes than
workgroups, so that a workgroup runs several."""
import ctypes as C
import functools
import importlib
import itertools
import re

import numpy as np
import pytest

import detect_model as dm
from conftest import load_pkg

pytestmark = pytest.mark.gpu

NBINS = (16, 18, 64, 100, 1024, 4096, 16384)
NROWS = (1, 3, 257, 2049)
MAX_CELLS = 2 ** 21
SHAPES = [(b, r) for b in NBINS for r in NROWS if b * r <= MAX_CELLS]
PARAMS = ((8, 1), (32, 2), (1024, 256))          # (train, guard); the last clips every window at 64 bins and leaves none at 16
MODES = ("ca", "go", "so")
GROUPING = tuple(itertools.product((1, 3), (0, 2, 70)))      # (min_width, max_gap)
FLOOR, SIGMA, THRESHOLD = -90.0, 2.0, 10.0       # the cloud; the threshold lies 5 sigma above a clean floor


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def X():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.detect")


def composite(row, rng):
    """One row with every kind of injection that fits: plateaus +25 dB of widths 1, 2, 3, 5, 64, 65, 200; plateaus at both ends of
    the row; pairs of plateaus 1, 2, 3 and 71 bins apart; plateaus across bins 60..70, 250..260, 1020..1030 (lane, wave and word
    boundaries); single NaN, -inf and +inf bins and a NaN inside a plateau."""
    n = len(row)
    hot = np.float32(FLOOR + 25.0)

    def plateau(start, width):
        if start >= 0 and start + width <= n:
            row[start:start + width] = hot + np.float32(0.25) * rng.integers(0, 4, width).astype(np.float32)
            return True
        return False

    cur = 4
    for width, gap in zip((1, 2, 3, 5, 64, 65, 200), (4, 9, 75, 5, 12, 80, 90)):
        plateau(cur, width)
        cur += width + gap
    for sep in (1, 2, 3, 71):
        plateau(cur, 3)
        plateau(cur + 3 + sep, 3)
        cur += 6 + sep + 40
    for start in (60, 250, 1020):
        plateau(start, 11)
    plateau(0, 2)
    plateau(n - 2, 2)
    for k, value in enumerate((np.nan, -np.inf, np.inf)):
        at = cur + 20 * k if cur + 60 < n else (5 + 3 * k) % n
        row[at] = value
    if plateau(cur + 80, 9):
        row[cur + 84] = np.nan
    elif n >= 64:
        row[30:39] = hot
        row[34] = np.nan


def cloud(seed, nrows, nbins):
    """A normal dB cloud, -90 dB with sigma 2.  Every third row carries injections, in turn: the composite row, an all-NaN row,
    an all -inf row, a constant row, a row whose every other bin is hot (nbins / 2 emissions), the composite row shifted by a
    random roll.  With three rows the one hot row is the every-other-bin row, so that the longest rows see it too."""
    rng = np.random.default_rng(seed)
    rows = (FLOOR + SIGMA * rng.standard_normal((nrows, nbins))).astype(np.float32)
    for i, r in enumerate(range(0, nrows, 3)):
        kind = (i + (4 if nrows == 3 else 0)) % 6
        if kind == 0:
            composite(rows[r], rng)
        elif kind == 1:
            rows[r] = np.nan
        elif kind == 2:
            rows[r] = -np.inf
        elif kind == 3:
            rows[r] = np.float32(FLOOR)
        elif kind == 4:
            rows[r, ::2] = np.float32(FLOOR + 25.0)
        else:
            composite(rows[r], rng)
            rows[r] = np.roll(rows[r], int(rng.integers(1, nbins)))
    return rows


@functools.lru_cache(maxsize=2)
def case_rows(nbins, nrows):
    rows = cloud(nbins * 7 + nrows, nrows, nbins)
    rows.setflags(write=False)
    return rows


def run_dev(X, torch, dev, nrows, nbins, cfg, capacity=1 << 20, want_floor=True, **kw):
    """One object, one detect_rows_dev call: dict(hits, seen, ev, total, count, floor, info)."""
    train, guard, mode, min_width, max_gap = cfg
    count = torch.full((nrows,), -7, dtype=torch.int32, device="cuda")
    floor = torch.full((nrows, nbins), 123.0, dtype=torch.float32, device="cuda") if want_floor else None
    det = X.SignalDetector(nbins, train, guard, THRESHOLD, mode=mode, min_width=min_width, max_gap=max_gap, capacity=capacity)
    det.detect_rows_dev(dev, nrows, row_count=count, floor=floor, **kw)
    hits, seen = det.hits()
    ev, total = det.emissions()
    info = det.kernel_info()
    det.close()
    return dict(hits=hits, seen=seen, ev=ev, total=total, count=count.cpu().numpy(),
                floor=floor.cpu().numpy() if want_floor else None, info=info)


def assert_same(got, want, nrows, capacity=1 << 20, base=0):
    assert got["hits"].dtype == np.int64 and got["seen"] == base + nrows
    assert np.array_equal(got["count"], want["count"]), "row_count"
    assert int(got["count"].sum()) == got["total"] == want["total"]
    assert np.array_equal(got["hits"], want["hits"]), "hits"
    ev, ref = got["ev"], want["all"][:capacity]
    assert ev.dtype == dm.EMISSION_DTYPE and len(ev) == len(ref)
    for name in dm.EMISSION_DTYPE.names:
        a, b = ev[name], ref[name]
        if name in ("peak_db", "floor_db"):
            a, b = a.view(np.int32), b.view(np.int32)
        assert np.array_equal(a, b), (name, a[:8], b[:8])
    if got["floor"] is not None:
        assert dm.floors_equal(got["floor"], want["floor"]), "floor line"
    if capacity >= want["total"]:
        assert int(got["hits"].sum()) >= int((ev["bin_hi"] - ev["bin_lo"] + 1).sum()) >= int(ev["ndet"].sum())
        assert int(got["hits"].sum()) == int((ev["bin_hi"] - ev["bin_lo"] + 1).sum())


def rows_per_wg(nbins):
    """One 16-byte load per lane up to 1024 bins, never fewer than 16 lanes per row."""
    lanes = 16
    while lanes < 256 and lanes * 4 < nbins:
        lanes *= 2
    return 256 // lanes


def configs_for(nbins, nrows, train, guard):
    """Every mode with every (min_width, max_gap) pair where the model is quick; on the large shapes every mode twice, the
    pairs taken in turn so that the three parameter sets together still see all six."""
    if nbins * nrows <= 2 ** 18:
        return [(train, guard, m, w, g) for m in MODES for w, g in GROUPING]
    first = PARAMS.index((train, guard)) * 2
    return [(train, guard, m, *GROUPING[(first + i + 3 * j) % 6]) for i, m in enumerate(MODES) for j in (0, 1)]


# ------------------------------------------------------------------------------------------ 1. against the model
@pytest.mark.parametrize("train,guard", PARAMS)
@pytest.mark.parametrize("nbins,nrows", SHAPES)
def test_emissions_hits_and_floor_match_the_model(X, torch_cuda, nbins, nrows, train, guard):
    rows = case_rows(nbins, nrows)
    dev = torch_cuda.from_numpy(np.array(rows)).cuda()
    totals = []
    for cfg in configs_for(nbins, nrows, train, guard):
        want = dm.detect(rows, train, guard, THRESHOLD, cfg[2], cfg[3], cfg[4], capacity=1 << 20)
        got = run_dev(X, torch_cuda, dev, nrows, nbins, cfg)
        assert_same(got, want, nrows)
        assert got["info"]["threads"] == 256 and got["info"]["grid"] >= 1
        assert got["info"]["vec"] == (1 if nbins % 4 == 0 else 0)
        assert got["info"]["rows_per_wg"] == rows_per_wg(nbins)
        totals.append((cfg[3], want["total"]))
    if nbins == 16 and train == 1024:
        assert not any(t for _, t in totals), "guard 256 leaves a 16-bin row no training cell"
    elif train <= 32 and nbins >= 64:
        assert all(t > 0 for w, t in totals if w == 1), "the injections must be found on the model alone"


def clustered(seed, nrows, nbins, block):
    """The cloud with its injections clustered: rows come in blocks of `block`, three blocks in four stay quiet, in the others
    every third row carries an injection as in cloud().  A workgroup that takes several blocks in turn then meets quiet blocks
    (nothing detected), noisy blocks (the walk, records, hits) and both orders of the two."""
    rng = np.random.default_rng(seed)
    rows = (FLOOR + SIGMA * rng.standard_normal((nrows, nbins))).astype(np.float32)
    noisy = rng.random(-(-nrows // block)) < 0.25
    kind = 0
    for blk in np.flatnonzero(noisy):
        for r in range(blk * block, min((blk + 1) * block, nrows), 3):
            kind = (kind + 1) % 6
            if kind == 0 or kind == 5:
                composite(rows[r], rng)
            elif kind == 1:
                rows[r] = np.nan
            elif kind == 2:
                rows[r] = -np.inf
            elif kind == 3:
                rows[r] = np.float32(FLOOR)
            else:
                rows[r, ::2] = np.float32(FLOOR + 25.0)
    return rows, noisy


@pytest.mark.parametrize("nbins,nrows", [(16, 131072), (18, 116508)])
def test_workgroups_that_run_several_passes_match_the_model(X, torch_cuda, nbins, nrows):
    """More passes than the launch has workgroups (the largest row counts the cell limit allows, at the two shortest rows, in
    the 16-byte and the 4-byte form): a workgroup reuses its LDS for pass after pass, and meets passes in which nothing is
    detected, passes whose detections are all dropped by min_width, and passes with emissions, in either order."""
    assert nbins * nrows <= MAX_CELLS
    block = rows_per_wg(nbins)
    rows, noisy = clustered(nbins + 5, nrows, nbins, block)
    dev = torch_cuda.from_numpy(rows).cuda()
    for cfg in ((8, 1, "ca", 1, 2), (8, 1, "so", 3, 0)):
        want = dm.detect(rows, cfg[0], cfg[1], THRESHOLD, cfg[2], cfg[3], cfg[4], capacity=1 << 20)
        per_block = np.add.reduceat(want["count"], np.arange(0, nrows, block))
        detected = np.logical_or.reduceat(want["det0"].any(axis=1), np.arange(0, nrows, block))
        assert (per_block > 0).sum() > 100 and (~detected).sum() > 100, "the case needs quiet and noisy passes"
        if cfg[3] == 3:
            assert (detected & (per_block == 0)).sum() > 10, "and passes whose every detection is too narrow"
        assert 0 < want["total"] <= 1 << 20
        got = run_dev(X, torch_cuda, dev, nrows, nbins, cfg)
        passes = -(-nrows // block)
        assert got["info"]["rows_per_wg"] == block and passes >= 1.5 * got["info"]["grid"], (passes, got["info"])
        assert_same(got, want, nrows)


# ------------------------------------------------------------------------------------------ 2. alignment and stride
@pytest.mark.parametrize("nbins", [4096, 1024, 64, 16])
def test_unaligned_base_and_odd_stride_give_the_same(X, torch_cuda, nbins):
    torch = torch_cuda
    nrows = 37
    rows = cloud(nbins + 1, nrows, nbins)
    cfg = (8, 1, "ca", 1, 2)
    want = dm.detect(rows, 8, 1, THRESHOLD, "ca", 1, 2, capacity=1 << 20)
    assert want["total"] > 0
    results = {}
    for name, offset, stride in (("aligned", 0, nbins), ("padded", 0, nbins + 4), ("odd stride", 0, nbins + 3),
                                 ("unaligned", 1, nbins + 4), ("unaligned odd", 1, nbins + 3)):
        padded = np.full(offset + nrows * stride, np.float32(40.0), dtype=np.float32)     # what lies between the rows must not be seen
        padded[offset:].reshape(nrows, stride)[:, :nbins] = rows
        dev = torch.from_numpy(padded).cuda()
        assert dev[offset:].data_ptr() % 16 == 4 * offset
        got = run_dev(X, torch, dev[offset:], nrows, nbins, cfg, row_stride=stride)
        assert got["info"]["vec"] == (1 if offset == 0 and stride % 4 == 0 else 0), name
        assert_same(got, want, nrows)
        results[name] = got
    a = results["aligned"]
    for name, b in results.items():
        assert np.array_equal(a["hits"], b["hits"]) and a["ev"].tobytes() == b["ev"].tobytes() and a["total"] == b["total"], name
        assert a["floor"].tobytes() == b["floor"].tobytes(), name


# ------------------------------------------------------------------------------------------ 3. accumulation
@pytest.mark.parametrize("nbins", [4096, 64])
def test_calls_accumulate_and_host_rows_equal_device_rows(X, torch_cuda, nbins):
    torch = torch_cuda
    nrows = 40
    rows = cloud(99 + nbins, nrows, nbins)
    dev = torch.from_numpy(rows).cuda()
    args = (32, 2, THRESHOLD, "go", 1, 2)
    want = dm.detect(rows, *args, capacity=1 << 20)
    assert want["total"] > 10
    make = lambda: X.SignalDetector(nbins, *args[:3], mode="go", min_width=1, max_gap=2, capacity=1 << 16)
    one, cut, host, based = make(), make(), make(), make()
    one.detect_rows_dev(dev)
    cut.detect_rows_dev(dev, 1)
    cut.detect_rows_dev(dev[1:], 7)
    cut.detect_rows_dev(dev[8:], nrows - 8)
    cut.detect_rows_dev(dev, 0)                               # a successful no-op
    host.detect_rows(rows[:9])
    host.detect_rows(rows[9:])
    host.detect_rows(rows[:0])
    based.set_row_base(1000)
    based.detect_rows_dev(dev, 9)
    based.set_row_base(5000)
    based.detect_rows(rows[9:])
    for det in (one, cut, host):
        hits, seen = det.hits()
        ev, total = det.emissions()
        assert seen == nrows and total == want["total"] and np.array_equal(hits, want["hits"])
        assert dm.emissions_equal(ev, want["all"])
        assert np.array_equal(det.occupancy(), want["hits"] / float(nrows))
    ev, total = based.emissions()
    hits, seen = based.hits()
    first = dm.detect(rows[:9], *args, capacity=1 << 20, row_base=1000)
    second = dm.detect(rows[9:], *args, capacity=1 << 20, row_base=5000)
    assert seen == 5000 + nrows - 9 and np.array_equal(hits, want["hits"]) and total == want["total"]
    assert dm.emissions_equal(ev, np.concatenate([first["all"], second["all"]]))
    for det in (one, cut, host, based):
        det.close()


# ------------------------------------------------------------------------------------------ 4. capacity, clear, reset
def test_capacity_keeps_the_first_records_and_clear_and_reset_re_arm(X, torch_cuda):
    torch = torch_cuda
    nbins, nrows = 64, 40
    rows = cloud(4, nrows, nbins)
    args = (8, 1, THRESHOLD, "ca", 1, 0)
    full = dm.detect(rows, *args, capacity=1 << 20)
    assert full["total"] >= 10
    dev = torch.from_numpy(rows).cuda()
    det = X.SignalDetector(nbins, 8, 1, THRESHOLD, capacity=5)
    det.detect_rows_dev(dev, 1)                               # the buffer fills inside the second call
    det.detect_rows_dev(dev[1:], nrows - 1)
    ev, total = det.emissions()
    hits, seen = det.hits()
    assert len(ev) == 5 and total == full["total"] and dm.emissions_equal(ev, full["all"][:5])
    assert np.array_equal(hits, full["hits"]) and seen == nrows
    det.clear_emissions()
    ev, total = det.emissions()
    assert len(ev) == 0 and total == 0
    assert np.array_equal(det.hits()[0], full["hits"]) and det.rows_seen == nrows     # hits and rows_seen stay
    det.detect_rows_dev(dev[3:], nrows - 3)
    again = dm.detect(rows[3:], *args, capacity=1 << 20, row_base=nrows)
    ev, total = det.emissions()
    assert dm.emissions_equal(ev, again["all"][:5]) and total == again["total"]
    det.reset()
    hits, seen = det.hits()
    ev, total = det.emissions()
    assert not hits.any() and seen == 0 and len(ev) == 0 and total == 0
    det.detect_rows(rows)                                     # numbered from 0 again
    assert dm.emissions_equal(det.emissions()[0], full["all"][:5]) and np.array_equal(det.hits()[0], full["hits"])
    det.close()


# ------------------------------------------------------------------------------------------ 5. set_params, merge
def test_set_params_and_merge_hits(X, torch_cuda):
    torch = torch_cuda
    nbins, nrows = 100, 40
    rows = cloud(7, nrows, nbins)
    dev = torch.from_numpy(rows).cuda()
    a = X.SignalDetector(nbins, 8, 1, THRESHOLD, capacity=1 << 16)
    a.detect_rows_dev(dev, 10)
    a.set_params(train=32, guard=2, threshold_db=6.0, mode="so", min_width=3, max_gap=2)       # no synchronisation in between
    a.detect_rows_dev(dev[10:], nrows - 10)
    first = dm.detect(rows[:10], 8, 1, THRESHOLD, "ca", 1, 0, capacity=1 << 20)
    second = dm.detect(rows[10:], 32, 2, 6.0, "so", 3, 2, capacity=1 << 20, row_base=10)
    hits, seen = a.hits()
    ev, total = a.emissions()
    assert seen == nrows and np.array_equal(hits, first["hits"] + second["hits"]) and second["total"] > 0
    assert total == first["total"] + second["total"]
    assert dm.emissions_equal(ev, np.concatenate([first["all"], second["all"]]))
    with pytest.raises(X.KsaError, match="train"):
        a.set_params(train=0)
    assert a.params[0] == 32
    # merge: b += a through the zero-copy view of a's hits
    b = X.SignalDetector(nbins, 8, 1, THRESHOLD)
    b.detect_rows(rows[:10])
    view = torch.as_tensor(a.hits_view(), device="cuda")
    assert view.dtype == torch.int64 and tuple(view.shape) == (nbins,)
    a.synchronize()
    assert np.array_equal(view.cpu().numpy(), hits)
    b.merge_hits_dev(view, rows_seen_add=nrows)
    got, seen = b.hits()
    assert np.array_equal(got, hits + first["hits"]) and seen == nrows + 10
    assert b.emissions()[1] == first["total"]                 # emission lists are not merged
    want = got.copy()                                         # 64-bit sums: merged with its own read-back it doubles 34 times
    for _ in range(34):
        back, _ = b.hits()
        b.merge_hits_dev(torch.from_numpy(back).cuda())
        want += want
    got, seen = b.hits()
    assert want.max() > 2 ** 33 and seen == nrows + 10 and np.array_equal(got, want)
    a.close(), b.close()


# ------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_have_their_own_text_and_change_nothing(X, torch_cuda):
    torch = torch_cuda
    lib = X.lib()
    texts = []

    def refused(rc):
        assert rc != 0
        text = lib.kse_last_error().decode()
        assert text
        texts.append(text)

    nbins = 64
    rows = cloud(3, 20, nbins)
    det = X.SignalDetector(nbins, 8, 1, THRESHOLD)
    det.detect_rows(rows)
    hits_before, seen_before = det.hits()
    ev_before, total_before = det.emissions()
    assert total_before > 0
    dev = torch.from_numpy(rows).cuda()
    other = torch.ones(nbins, dtype=torch.int64, device="cuda")
    h, p, hp = det._h, C.c_void_p(dev.data_ptr()), rows.ctypes.data_as(C.c_void_p)
    n64 = C.c_int64()
    refused(lib.kse_detect_rows_dev(h, None, nbins, 20, None, None))
    refused(lib.kse_detect_rows_dev(h, p, nbins, -1, None, None))
    refused(lib.kse_detect_rows_dev(h, p, nbins - 1, 20, None, None))
    refused(lib.kse_detect_rows_dev(None, p, nbins, 20, None, None))
    refused(lib.kse_detect_rows(h, None, 20))
    refused(lib.kse_detect_rows(h, hp, -1))
    refused(lib.kse_set_row_base(h, -1))
    refused(lib.kse_read_hits(h, None, None))
    refused(lib.kse_read_emissions(h, None, -1, C.byref(n64), C.byref(n64)))
    refused(lib.kse_read_emissions(h, None, 0, None, None))
    refused(lib.kse_hits_dev(h, None))
    refused(lib.kse_emissions_dev(h, None, None))
    refused(lib.kse_merge_hits_dev(h, None, 0))
    refused(lib.kse_merge_hits_dev(h, C.c_void_p(other.data_ptr()), -1))
    refused(lib.kse_set_params(h, 0, 1, 10.0, 0, 1, 0))
    refused(lib.kse_set_params(h, 8, 257, 10.0, 0, 1, 0))
    refused(lib.kse_set_params(h, 8, 1, float("nan"), 0, 1, 0))
    refused(lib.kse_set_params(h, 8, 1, 10.0, 3, 1, 0))
    refused(lib.kse_set_params(h, 8, 1, 10.0, 0, 65, 0))
    refused(lib.kse_set_params(h, 8, 1, 10.0, 0, 1, 1025))
    assert len({re.sub(r"-?[0-9.]+", "#", t) for t in texts}) >= 18, texts
    with pytest.raises(X.KsaError, match="row_stride"):
        det.detect_rows_dev(dev, 20, row_stride=nbins - 1)
    with pytest.raises(X.KsaError):
        det.detect_rows(rows[:, :nbins - 1])
    hits_after, seen_after = det.hits()
    ev_after, total_after = det.emissions()
    det.detect_rows(rows[:3])                                 # the refused set_params calls left the parameters alone
    assert det.emissions()[1] == total_before + dm.detect(rows[:3], 8, 1, THRESHOLD)["total"]
    p2, tot = C.c_void_p(), C.c_void_p()
    assert lib.kse_emissions_dev(h, C.byref(p2), C.byref(tot)) == 0 and p2.value and tot.value
    det.close()
    assert np.array_equal(hits_after, hits_before) and seen_after == seen_before == 20
    assert ev_after.tobytes() == ev_before.tobytes() and total_after == total_before


# ------------------------------------------------------------------------------------------ 7. behind the engine
def test_rows_of_the_engine_are_searched_in_stream_order(ksa, X, torch_cuda):
    torch = torch_cuda
    n, frames = 4096, 8
    rng = np.random.default_rng(11)
    eng = ksa.SpectrumEngine(n, non_overlap=0.5, window="hanning", max_frames=frames)
    full = eng.full_size
    x = (rng.standard_normal((frames, full)) + 1j * rng.standard_normal((frames, full))).astype(np.complex64) * 0.05
    x += np.exp(2j * np.pi * 0.123 * np.arange(full)).astype(np.complex64)
    dev = torch.view_as_real(torch.from_numpy(x)).cuda()
    buf = torch.full((frames, n), float("nan"), dtype=torch.float32, device="cuda")
    count = torch.zeros(frames, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    det = X.SignalDetector(n, 32, 2, THRESHOLD, mode="ca", min_width=1, max_gap=2)
    torch.cuda.synchronize()
    eng.set_stream(stream.cuda_stream)
    det.set_stream(stream.cuda_stream)
    eng.frames_dev(dev, ksa.FMT_C64, frames, cur_db=buf)
    det.detect_rows_dev(buf, frames, row_count=count)         # no synchronisation between the two: zero-copy over cur_db
    ev, total = det.emissions()
    hits, seen = det.hits()
    rows = buf.cpu().numpy()
    assert seen == frames and not np.isnan(rows).any()
    want = dm.detect(rows, 32, 2, THRESHOLD, "ca", 1, 2, capacity=1 << 20)
    assert dm.emissions_equal(ev, want["all"]) and total == want["total"] and np.array_equal(hits, want["hits"])
    assert np.array_equal(count.cpu().numpy(), want["count"])
    tone = int(np.argmax(rows[0]))
    assert np.all(np.argmax(rows, axis=1) == tone)
    for r in range(frames):
        mine = ev[ev["row"] == r]
        assert np.any((mine["bin_lo"] <= tone) & (tone <= mine["bin_hi"]) & (mine["peak_bin"] == tone)), r
    assert hits[tone] == frames and det.occupancy()[tone] == 1.0
    det.close()
    eng.close()


# ------------------------------------------------------------------------------------------ 8. the command line
def test_cli_detect_reports_and_leaves_the_state_alone(ksa, X, torch_cuda, tmp_path, capsys):
    K = importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")
    sources = importlib.import_module("prgs-sdr-kspecanal_amd.sources")
    n, frames = 512, 21                                       # 21 = 2 batches of 8 and one of 5
    common = ["zeroSpan", "fftSize", str(n), "window", "hanning", "source", "synth", "bPltLevels", "false", "bPltHeatMap", "false",
              "prgLoopCnt", str(frames)]
    base = K.handle_args({}, common)
    full = base["fullSize"]
    # what an engine of the same configuration returns for the same blocks
    src = sources.SyntheticSdr()
    src.sample_rate, src.center_freq, src.gain = base["samplingRate"], base["centerFreq"], base["gain"]
    src.read_samples(16 * 1024)                               # the settle samples sdr_setup discards
    blocks = np.array([K.sdr_read(src, full) for _ in range(frames)])
    eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=base["curScanNonOverlap"], window=base["theWin"],
                             cumu_mode=base["curScanCumuMode"], gain=base["gain"], min_amp=base["minAmp4Clip"],
                             xres=base["xRes"], max_frames=frames)
    db, _ = eng.frames(blocks, cur_db=True)
    eng.close()
    want = dm.detect(db, 16, 2, 8.0, "go", 1, 3, capacity=1 << 20)
    assert want["total"] > 6 and np.all(want["count"] > 0), "the synthetic source's tones must be found on the model alone"

    def run(extra):
        K.sdr_curscan = K._gpu_curscan
        capsys.readouterr()
        d = K.main(common + extra)
        return d, capsys.readouterr().out

    key = "16:2:8:mode=go:maxGap=3:events=6"
    for batch in ("8", "1"):
        plain, _ = run(["frameBatch", batch])
        save = tmp_path / ("e%s.npz" % batch)
        d, out = run(["frameBatch", batch, "detect", key, "detectSave", str(save)])
        z = np.load(save)
        assert sorted(z.files) == ["center_hz", "emissions", "emissions_total", "guard", "hits", "max_gap", "min_width", "mode",
                                   "rows_seen", "threshold_db", "train", "width_hz"]
        assert dm.emissions_equal(z["emissions"], want["all"][:6]) and int(z["emissions_total"]) == want["total"], batch
        assert np.array_equal(z["hits"], want["hits"]) and int(z["rows_seen"]) == frames
        assert (int(z["train"]), int(z["guard"]), float(z["threshold_db"]), str(z["mode"]), int(z["min_width"]),
                int(z["max_gap"])) == (16, 2, 8.0, "go", 1, 3)
        center, width = dm.emission_freqs(want["all"][:6], d["freqs"])
        assert np.array_equal(z["center_hz"], center) and np.array_equal(z["width_hz"], width) and np.all(width > 0)
        assert dm.emissions_equal(d["detectEmissions"], want["all"][:6]) and d["detectEmissionsTotal"] == want["total"]
        assert np.array_equal(d["detectHits"], want["hits"]) and d["detectRows"] == frames
        busiest = int(np.argmax(want["hits"]))
        assert re.search(r"^INFO:zero_span: detect rows \[%d\], emissions stored \[6\] / total \[%d\], highest occupancy \[%.6f\] at bin \[%d\]"
                         % (frames, want["total"], want["hits"][busiest] / frames, busiest), out, flags=re.M)
        for k in ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg", "fftHM"):
            assert np.array_equal(d[k], plain[k]), (batch, k)              # bit for bit
        assert d["fftHMIndex"] == plain["fftHMIndex"] == frames % 128
    # with the density, the mask and the zoom keys: one run
    d, _ = run(["frameBatch", "8", "detect", key, "density", "64:-120:0", "mask", "flat:-20"])
    assert dm.emissions_equal(d["detectEmissions"], want["all"][:6]) and d["densityRows"] == frames and d["maskRows"] == frames
    d, out = run(["frameBatch", "8", "detect", key, "zoom", "4"])
    assert d["detectRows"] == frames and "detect rows [%d]" % frames in out
