"""The frequency-mask trigger on the GPU against its float32 model (tests/mask_model.py).  Every comparison is exact:
np.array_equal on the hits, and on every field of the event records (the excess by its bits).  Shapes are the smallest at which
the check pass takes each of its paths: strips narrower than a wave (several rows per wave), one strip, several strips, a short
last strip, one and several chunks of rows, 16-byte and 4-byte loads, one and several workgroups of the compaction."""
import ctypes as C
import functools
import importlib
import re

import numpy as np
import pytest

import mask_model as mm
from conftest import load_pkg

pytestmark = pytest.mark.gpu

NBINS = (16, 64, 4096)
NROWS = (1, 3, 257, 5000)
FLOOR, SIGMA = -90.0, 2.0            # the cloud; the lines lie 7 sigma and more away, so only injected values cross them


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def M():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.mask")


def lines_for(nbins, with_lower):
    """Lines that differ from bin to bin: upper -75 .. -73.5 dB, lower -105 .. -107 dB (or none)."""
    b = np.arange(nbins)
    up = (-75.0 + (b % 7) * 0.25).astype(np.float32)
    lo = (-105.0 - (b % 5) * 0.5).astype(np.float32) if with_lower else None
    return up, lo


def cloud(seed, nrows, nbins, up, lo):
    """A normal dB cloud that crosses no line, with special values injected into every third row (the others stay quiet):
    -inf, +inf, NaN, values exactly on a line and one float32 ulp either side of it, values 10 dB beyond it.  Row 0 always holds
    four bins over the upper line.  No excess is subnormal: values and lines are of magnitude 64..128, so two that differ do so by
    at least 2^-17."""
    rng = np.random.default_rng(seed)
    rows = (FLOOR + SIGMA * rng.standard_normal((nrows, nbins))).astype(np.float32)
    low = lo if lo is not None else np.full(nbins, -105.0, dtype=np.float32)
    inf32 = np.float32(np.inf)
    table = np.stack([np.full(nbins, -inf32), np.full(nbins, inf32), np.full(nbins, np.float32(np.nan)),
                      up, np.nextafter(up, inf32), np.nextafter(up, -inf32), low, np.nextafter(low, -inf32),
                      np.nextafter(low, inf32), up + np.float32(10), low - np.float32(10)]).astype(np.float32)
    hot = np.arange(0, nrows, 3)
    k = max(4, nbins // 16)
    bins = rng.integers(0, nbins, size=(len(hot), k))
    kinds = rng.integers(0, len(table), size=(len(hot), k))
    rows[hot[:, None], bins] = table[kinds, bins]
    rows[0, 1:5] = [up[1] + np.float32(10), np.nextafter(up[2], inf32), inf32, up[4] + np.float32(20)]
    return rows


@functools.lru_cache(maxsize=2)
def case_rows(nbins, nrows, with_lower):
    up, lo = lines_for(nbins, with_lower)
    rows = cloud(nbins * 5 + nrows + (1 if with_lower else 0), max(nrows, 2), nbins, up, lo)
    rows.setflags(write=False)
    return rows, up, lo


def run_dev(M, torch, rows, up, lo, min_bins=1, capacity=4096, row_base=None):
    """One object, one check_rows_dev call: (hits, rows_seen, events, total, row_event, kernel_info)."""
    dev = torch.from_numpy(np.array(rows, dtype=np.float32)).cuda()
    flag = torch.full((len(rows),), 7, dtype=torch.uint8, device="cuda")
    m = M.SpectrumMask(rows.shape[1], up, lo, min_bins=min_bins, capacity=capacity)
    if row_base is not None:
        m.set_row_base(row_base)
    m.check_rows_dev(dev, row_event=flag)
    hits, seen = m.hits()
    ev, total = m.events()
    info = m.kernel_info()
    m.close()
    return hits, seen, ev, total, flag.cpu().numpy(), info


def assert_same(got, want, nrows, min_bins, capacity, base=0):
    hits, seen, ev, total, flag, _ = got
    assert hits.dtype == np.int64 and seen == base + nrows
    for k, name in enumerate(("over", "under", "nan")):
        assert np.array_equal(hits[k], want["hits"][k]), name
    assert total == want["total"]
    assert np.array_equal(flag, want["event"].astype(np.uint8)), "row_event"
    assert ev.dtype == mm.EVENT_DTYPE and len(ev) == len(want["events"])
    for name in mm.EVENT_DTYPE.names:
        a, b = ev[name], want["events"][name]
        if name == "peak_excess":
            a, b = a.view(np.int32), b.view(np.int32)
        assert np.array_equal(a, b), (name, a[:8], b[:8])
    assert np.all(np.diff(ev["row"]) > 0)
    if min_bins == 1 and total <= capacity:
        for k, name in enumerate(("nover", "nunder", "nnan")):
            assert hits[k].sum() == ev[name].sum(), name


# ------------------------------------------------------------------------------------------ 1. against the model
@pytest.mark.parametrize("min_bins", [1, 3])
@pytest.mark.parametrize("with_lower", [True, False])
@pytest.mark.parametrize("nrows", NROWS)
@pytest.mark.parametrize("nbins", NBINS)
def test_hits_and_events_match_the_model(M, torch_cuda, nbins, nrows, with_lower, min_bins):
    rows, up, lo = case_rows(nbins, nrows, with_lower)
    whole = mm.check(rows, up, lo, min_bins)
    assert whole["event"].any() and not whole["event"].all(), "the case needs an event row and a quiet row"
    assert whole["event"][0] and not whole["event"][1]
    if nrows == 1:                                            # one row cannot be both: the event row, then the quiet row
        for r in (0, 1):
            want = mm.check(rows[r:r + 1], up, lo, min_bins)
            assert_same(run_dev(M, torch_cuda, rows[r:r + 1], up, lo, min_bins), want, 1, min_bins, 4096)
        return
    got = run_dev(M, torch_cuda, rows, up, lo, min_bins)
    assert_same(got, whole, nrows, min_bins, 4096)
    assert got[5]["threads"] == 256 and got[5]["grid"] >= 1 and got[5]["vec"] == 1


@pytest.mark.parametrize("nbins,nrows", [(18, 37), (48, 37), (2400, 37), (2400, 300)])
def test_sizes_that_are_no_power_of_two(M, torch_cuda, nbins, nrows):
    """A row that is no multiple of four floats (the 4-byte form even from an aligned buffer), a strip that is no power of two,
    a short last strip."""
    up, lo = lines_for(nbins, True)
    rows = cloud(nbins + nrows, nrows, nbins, up, lo)
    want = mm.check(rows, up, lo, 1)
    assert want["event"].any() and not want["event"].all()
    got = run_dev(M, torch_cuda, rows, up, lo)
    assert_same(got, want, nrows, 1, 4096)
    assert got[5]["vec"] == (1 if nbins % 4 == 0 else 0)


# ------------------------------------------------------------------------------------------ 2. alignment and stride
@pytest.mark.parametrize("nbins", [4096, 2400, 64, 16])
def test_unaligned_base_and_odd_stride_give_the_same(M, torch_cuda, nbins):
    torch = torch_cuda
    nrows = 257
    up, lo = lines_for(nbins, True)
    rows = cloud(nbins + 1, nrows, nbins, up, lo)
    want = mm.check(rows, up, lo, 1)
    assert want["event"].any() and not want["event"].all()
    results = {}
    for name, offset, stride in (("aligned", 0, nbins), ("padded", 0, nbins + 4), ("odd stride", 0, nbins + 3),
                                 ("unaligned", 1, nbins + 4), ("unaligned odd", 1, nbins + 3)):
        padded = np.full(offset + nrows * stride, np.nan, dtype=np.float32)      # what lies between the rows must not be seen
        padded[offset:].reshape(nrows, stride)[:, :nbins] = rows
        dev = torch.from_numpy(padded).cuda()
        flag = torch.zeros(nrows, dtype=torch.uint8, device="cuda")
        m = M.SpectrumMask(nbins, up, lo)
        m.check_rows_dev(dev[offset:], nrows, row_stride=stride, row_event=flag)
        assert dev[offset:].data_ptr() % 16 == 4 * offset
        got = m.hits() + m.events() + (flag.cpu().numpy(), m.kernel_info())
        m.close()
        assert got[5]["vec"] == (1 if offset == 0 and stride % 4 == 0 else 0), name
        assert_same(got, want, nrows, 1, 4096)
        results[name] = got
    a = results["aligned"]
    for name, b in results.items():
        assert np.array_equal(a[0], b[0]) and a[2].tobytes() == b[2].tobytes() and a[3] == b[3], name


# ------------------------------------------------------------------------------------------ 3. accumulation
@pytest.mark.parametrize("nbins", [4096, 64])
def test_calls_accumulate_and_host_rows_equal_device_rows(M, torch_cuda, nbins):
    torch = torch_cuda
    up, lo = lines_for(nbins, True)
    rows = cloud(99 + nbins, 257, nbins, up, lo)
    dev = torch.from_numpy(rows).cuda()
    want = mm.check(rows, up, lo, 1)
    one = M.SpectrumMask(nbins, up, lo)
    one.check_rows_dev(dev)
    three = M.SpectrumMask(nbins, up, lo)
    three.check_rows_dev(dev, 100)
    three.check_rows_dev(dev[100:], 3)
    three.check_rows_dev(dev[103:], 154)
    three.check_rows_dev(dev, 0)                              # a successful no-op
    host = M.SpectrumMask(nbins, up, lo)
    host.check_rows(rows[:100])
    host.check_rows(rows[100:])
    host.check_rows(rows[:0])
    based = M.SpectrumMask(nbins, up, lo)
    based.set_row_base(1000)
    based.check_rows_dev(dev, 57)
    based.set_row_base(5000)
    based.check_rows(rows[57:])
    for m in (one, three, host):
        hits, seen = m.hits()
        ev, total = m.events()
        assert seen == 257 and total == want["total"] and np.array_equal(hits, want["hits"])
        assert mm.events_equal(ev, want["events"])
        assert np.array_equal(m.occupancy(), (want["hits"][0] + want["hits"][1]) / 257.0)
    ev, total = based.events()
    hits, seen = based.hits()
    first, second = mm.check(rows[:57], up, lo, 1, row_base=1000), mm.check(rows[57:], up, lo, 1, row_base=5000)
    assert seen == 5200 and np.array_equal(hits, want["hits"])
    assert mm.events_equal(ev, np.concatenate([first["events"], second["events"]])) and total == want["total"]
    for m in (one, three, host, based):
        m.close()


# ------------------------------------------------------------------------------------------ 4. capacity
def test_capacity_keeps_the_first_events_and_clear_re_arms(M, torch_cuda):
    torch = torch_cuda
    nbins, nrows = 64, 257
    up, lo = lines_for(nbins, True)
    rows = cloud(4, nrows, nbins, up, lo)
    want = mm.check(rows, up, lo, 1, capacity=4)
    full = mm.check(rows, up, lo, 1)
    assert full["total"] >= 10
    dev = torch.from_numpy(rows).cuda()
    m = M.SpectrumMask(nbins, up, lo, capacity=4)
    m.check_rows_dev(dev, 100)
    m.check_rows_dev(dev[100:], 157)
    ev, total = m.events()
    hits, seen = m.hits()
    assert len(ev) == 4 and total == full["total"] and mm.events_equal(ev, want["events"]) and mm.events_equal(ev, full["events"][:4])
    assert np.array_equal(hits, full["hits"]) and seen == nrows
    m.clear_events()
    ev, total = m.events()
    assert len(ev) == 0 and total == 0
    assert np.array_equal(m.hits()[0], full["hits"]) and m.rows_seen == nrows       # hits and rows_seen stay
    m.check_rows_dev(dev[100:], 157)
    again = mm.check(rows[100:], up, lo, 1, capacity=4, row_base=nrows)
    ev, total = m.events()
    assert mm.events_equal(ev, again["events"]) and total == again["total"]
    m.close()


# ------------------------------------------------------------------------------------------ 5. past one chunk
def test_counters_and_order_past_65536_rows(M, torch_cuda):
    torch = torch_cuda
    nrows, nbins, cap = 70000, 16, 100
    up = np.full(nbins, -50.0, dtype=np.float32)
    loud = torch.full((nrows, nbins), -40.0, dtype=torch.float32, device="cuda")
    flag = torch.zeros(nrows, dtype=torch.uint8, device="cuda")
    m = M.SpectrumMask(nbins, up, capacity=cap)
    m.check_rows_dev(loud, row_event=flag)
    hits, seen = m.hits()
    ev, total = m.events()
    assert seen == nrows and total == nrows and hits[0, 0] > 2 ** 16
    assert np.array_equal(hits, np.stack([np.full(nbins, nrows), np.zeros(nbins), np.zeros(nbins)]).astype(np.int64))
    assert np.array_equal(ev["row"], np.arange(cap)) and np.all(ev["nover"] == nbins) and np.all(ev["peak_bin"] == 0)
    assert np.all(ev["peak_excess"] == np.float32(10.0)) and np.all(ev["peak_kind"] == 0)
    assert bool(flag.all())
    assert np.array_equal(m.occupancy(), np.ones(nbins))
    m.reset()
    quiet = torch.full((nrows, nbins), -60.0, dtype=torch.float32, device="cuda")
    m.check_rows_dev(quiet, row_event=flag)
    hits, seen = m.hits()
    ev, total = m.events()
    m.close()
    assert seen == nrows and not hits.any() and total == 0 and len(ev) == 0 and not bool(flag.any())


# ------------------------------------------------------------------------------------------ 6. peak ties across strips
def test_peak_ties_across_strips_go_to_the_lowest_bin(M, torch_cuda):
    nbins = 4096
    up, lo = np.full(nbins, -50.0, dtype=np.float32), np.full(nbins, -120.0, dtype=np.float32)
    rows = np.full((3, nbins), -100.0, dtype=np.float32)
    rows[0, [5, 1500, 4090]] = -37.5
    rows[1, [5, 1500]] = -37.5
    rows[1, 4090] = np.inf
    rows[2, 1500], rows[2, 3000] = -132.5, -37.5              # under and over by the same 12.5 dB: the lower bin, an under
    want = mm.check(rows, up, lo, 1)
    assert want["peak_bin"].tolist() == [5, 4090, 1500] and want["peak_kind"].tolist() == [0, 0, 1]
    for form in ("vec", "scalar"):
        if form == "vec":
            got = run_dev(M, torch_cuda, rows, up, lo)
        else:
            torch = torch_cuda
            padded = np.full(1 + 3 * (nbins + 1), np.nan, dtype=np.float32)
            padded[1:].reshape(3, nbins + 1)[:, :nbins] = rows
            dev = torch.from_numpy(padded).cuda()
            flag = torch.zeros(3, dtype=torch.uint8, device="cuda")
            m = M.SpectrumMask(nbins, up, lo)
            m.check_rows_dev(dev[1:], 3, row_stride=nbins + 1, row_event=flag)
            got = m.hits() + m.events() + (flag.cpu().numpy(), m.kernel_info())
            m.close()
        assert got[5]["vec"] == (1 if form == "vec" else 0)
        assert_same(got, want, 3, 1, 4096)
        assert got[2]["peak_bin"].tolist() == [5, 4090, 1500]
        assert got[2]["peak_excess"].tolist() == [12.5, np.inf, 12.5]


# ------------------------------------------------------------------------------------------ 7. set_mask, merge, reset
def test_set_mask_merge_reset(M, torch_cuda):
    torch = torch_cuda
    nbins = 64
    up, lo = lines_for(nbins, True)
    rows = cloud(7, 257, nbins, up, lo)
    dev = torch.from_numpy(rows).cuda()
    a = M.SpectrumMask(nbins, up, lo)
    a.check_rows_dev(dev, 100)
    up2 = np.full(nbins, FLOOR, dtype=np.float32)             # the cloud's own floor: about every other bin is over
    a.set_mask(up2)                                           # and no lower line any more
    a.check_rows_dev(dev[100:], 157)
    first, second = mm.check(rows[:100], up, lo, 1), mm.check(rows[100:], up2, None, 1, row_base=100)
    hits, seen = a.hits()
    ev, total = a.events()
    assert seen == 257 and np.array_equal(hits, first["hits"] + second["hits"]) and second["hits"][0].sum() > 1000
    assert total == first["total"] + second["total"]
    assert mm.events_equal(ev, np.concatenate([first["events"], second["events"]])[:4096])
    # merge: b += a through the zero-copy view of a's hits
    b = M.SpectrumMask(nbins, up, lo)
    b.check_rows(rows[:100])
    view = torch.as_tensor(a.hits_view(), device="cuda")
    assert view.dtype == torch.int64 and tuple(view.shape) == (3, nbins)
    a.synchronize()
    assert np.array_equal(view.cpu().numpy(), hits)
    b.merge_hits_dev(view, rows_seen_add=257)
    got, seen = b.hits()
    assert np.array_equal(got, hits + first["hits"]) and seen == 357
    assert b.events()[1] == first["total"]                    # event lists are not merged
    # 64-bit sums: an object's own read-back merged 34 times doubles it 34 times
    want = got.copy()
    for _ in range(34):
        back, _ = b.hits()
        b.merge_hits_dev(torch.from_numpy(back).cuda())
        want += want
    got, seen = b.hits()
    assert want.max() > 2 ** 33 and seen == 357 and np.array_equal(got, want)
    b.reset()
    got, seen = b.hits()
    ev, total = b.events()
    assert not got.any() and seen == 0 and len(ev) == 0 and total == 0
    b.check_rows(rows[:100])                                  # numbered from 0 again
    assert mm.events_equal(b.events()[0], first["events"])
    a.close(), b.close()


# ------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_have_their_own_text_and_change_nothing(M, torch_cuda):
    torch = torch_cuda
    lib = M.lib()
    texts = []

    def refused(rc):
        assert rc != 0
        text = lib.ksm_last_error().decode()
        assert text
        texts.append(text)

    nbins = 64
    up, lo = lines_for(nbins, True)
    rows = cloud(3, 20, nbins, up, lo)
    m = M.SpectrumMask(nbins, up, lo)
    m.check_rows(rows)
    hits_before, seen_before = m.hits()
    ev_before, total_before = m.events()
    assert total_before > 0
    dev = torch.from_numpy(rows).cuda()
    other = torch.ones((3, nbins), dtype=torch.int64, device="cuda")
    h, p, hp = m._h, C.c_void_p(dev.data_ptr()), rows.ctypes.data_as(C.c_void_p)
    n64 = C.c_int64()
    refused(lib.ksm_check_rows_dev(h, None, nbins, 20, None))
    refused(lib.ksm_check_rows_dev(h, p, nbins, -1, None))
    refused(lib.ksm_check_rows_dev(h, p, nbins - 1, 20, None))
    refused(lib.ksm_check_rows_dev(None, p, nbins, 20, None))
    refused(lib.ksm_check_rows(h, None, 20))
    refused(lib.ksm_check_rows(h, hp, -1))
    refused(lib.ksm_set_row_base(h, -1))
    refused(lib.ksm_read_hits(h, None, None))
    refused(lib.ksm_read_events(h, None, -1, C.byref(n64), C.byref(n64)))
    refused(lib.ksm_read_events(h, None, 0, None, None))
    refused(lib.ksm_hits_dev(h, None))
    refused(lib.ksm_events_dev(h, None, None))
    refused(lib.ksm_merge_hits_dev(h, None, 0))
    refused(lib.ksm_merge_hits_dev(h, C.c_void_p(other.data_ptr()), -1))
    refused(lib.ksm_set_mask(h, None, None))
    bad = up.copy()
    bad[9] = np.nan
    refused(lib.ksm_set_mask(h, bad.ctypes.data_as(C.c_void_p), None))
    refused(lib.ksm_set_mask(h, lo.ctypes.data_as(C.c_void_p), up.ctypes.data_as(C.c_void_p)))      # lower above upper
    refused(lib.ksm_reset(None))
    refused(lib.ksm_clear_events(None))
    refused(lib.ksm_set_stream(None, None))
    assert len({re.sub(r"-?[0-9.]+", "#", t) for t in texts}) >= 14, texts
    with pytest.raises(M.KsaError, match="row_stride"):
        m.check_rows_dev(dev, 20, row_stride=nbins - 1)
    with pytest.raises(M.KsaError):
        m.check_rows(rows[:, :nbins - 1])
    with pytest.raises(M.KsaError, match="NaN"):
        m.set_mask(bad)
    hits_after, seen_after = m.hits()
    ev_after, total_after = m.events()
    m.check_rows(rows[:1])                                    # the refused set_mask calls left the lines alone
    assert m.events()[1] == total_before + 1
    m.close()
    assert np.array_equal(hits_after, hits_before) and seen_after == seen_before == 20
    assert ev_after.tobytes() == ev_before.tobytes() and total_after == total_before


# ------------------------------------------------------------------------------------------ 9. behind the engine
def test_rows_of_the_engine_are_checked_in_stream_order(ksa, M, torch_cuda):
    torch = torch_cuda
    n, frames = 512, 64
    planted = [3, 17, 18, 40, 63]
    rng = np.random.default_rng(11)
    eng = ksa.SpectrumEngine(n, non_overlap=0.5, window="hanning", max_frames=frames)
    full = eng.full_size

    def iq(tone_frames):
        x = (rng.standard_normal((frames, full)) + 1j * rng.standard_normal((frames, full))).astype(np.complex64) * 0.05
        for f in tone_frames:
            x[f] += np.exp(2j * np.pi * 0.123 * np.arange(full)).astype(np.complex64)
        return torch.view_as_real(torch.from_numpy(x)).cuda()

    quiet_db, _ = eng.frames(torch.view_as_complex(iq([])).cpu().numpy(), cur_db=True)
    eng.reset()
    upper = M.learn_mask(quiet_db, 6.0)
    assert np.array_equal(upper, mm.learn_mask(quiet_db, 6.0)) and np.isfinite(upper).all()
    dev = iq(planted)
    buf = torch.full((frames, n), float("nan"), dtype=torch.float32, device="cuda")
    flag = torch.zeros(frames, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    mask = M.SpectrumMask(n, upper)
    torch.cuda.synchronize()
    eng.set_stream(stream.cuda_stream)
    mask.set_stream(stream.cuda_stream)
    eng.frames_dev(dev, ksa.FMT_C64, frames, cur_db=buf)
    mask.check_rows_dev(buf, frames, row_event=flag)          # no synchronisation between the two
    ev, total = mask.events()
    hits, seen = mask.hits()
    rows = buf.cpu().numpy()
    assert seen == frames and not np.isnan(rows).any()
    want = mm.check(rows, upper, None, 1)
    assert want["events"]["row"].tolist() == planted, "tone level and margin must single out the planted frames on the model alone"
    assert mm.events_equal(ev, want["events"]) and total == len(planted)
    assert ev["row"].tolist() == planted and np.array_equal(hits, want["hits"])
    assert np.flatnonzero(flag.cpu().numpy()).tolist() == planted
    assert np.all(ev["peak_kind"] == 0) and np.all(ev["peak_excess"] > 6.0)
    mask.close()
    eng.close()


# ------------------------------------------------------------------------------------------ 10. the command line
def test_cli_mask_learns_reports_and_leaves_the_state_alone(ksa, M, torch_cuda, tmp_path, capsys):
    K = importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")
    sources = importlib.import_module("prgs-sdr-kspecanal_amd.sources")
    n, frames, learn = 512, 21, 5                             # 21 = 2 batches of 8 and one of 5; the boundary lies inside the first
    bursts = [7, 8, 15, 20]
    base = K.handle_args({}, ["zeroSpan", "fftSize", str(n), "iqFormat", "u8"])
    full = base["fullSize"]
    settle = 16 * 1024
    rng = np.random.default_rng(2025)
    t = np.arange(settle + frames * full)
    x = 0.4 * np.exp(2j * np.pi * 0.21 * t) + 0.05 * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
    for f in bursts:
        s = slice(settle + f * full, settle + (f + 1) * full)
        x[s] += 0.3 * np.exp(2j * np.pi * 0.37 * t[s])
    raw = np.empty(2 * t.size, dtype=np.uint8)
    raw[0::2] = np.clip(np.round(x.real * 127.5 + 127.5), 0, 255)
    raw[1::2] = np.clip(np.round(x.imag * 127.5 + 127.5), 0, 255)
    path = tmp_path / "cap_u8.bin"
    raw.tofile(path)
    common = ["zeroSpan", "fftSize", str(n), "iqFormat", "u8", "source", "file:%s" % path, "bPltLevels", "false",
              "bPltHeatMap", "false", "prgLoopCnt", str(frames)]

    # what an engine of the same configuration returns for the same blocks
    src = sources.FileSdr(str(path), iq_format="u8")
    src.read_samples(settle)                                  # the settle samples sdr_setup discards
    blocks = np.array([K.sdr_read(src, full, raw=True) for _ in range(frames)])
    src.close()
    eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=base["curScanNonOverlap"], window=base["theWin"],
                             cumu_mode=base["curScanCumuMode"], gain=base["gain"], min_amp=base["minAmp4Clip"],
                             xres=base["xRes"], max_frames=frames)
    db, _ = eng.frames(blocks, cur_db=True)
    eng.close()
    upper = mm.learn_mask(db[:learn], 6.0)
    want = mm.check(db[learn:], upper, None, 1, capacity=3, row_base=learn)
    assert mm.check(db[learn:], upper, None, 1, row_base=learn)["events"]["row"].tolist() == bursts
    assert want["events"]["row"].tolist() == bursts[:3] and want["total"] == len(bursts)

    def run(extra):
        K.sdr_curscan = K._gpu_curscan
        capsys.readouterr()
        d = K.main(common + extra)
        return d, capsys.readouterr().out

    for batch in ("8", "1"):
        plain, _ = run(["frameBatch", batch])
        save = tmp_path / ("m%s.npz" % batch)
        d, out = run(["frameBatch", batch, "mask", "learn:%d:6:events=3" % learn, "maskSave", str(save)])
        z = np.load(save)
        assert sorted(z.files) == ["event_rows", "events", "events_total", "hits", "lower", "rows_seen", "upper"]
        assert mm.events_equal(z["events"], want["events"]) and int(z["events_total"]) == len(bursts), batch
        assert np.array_equal(z["hits"], want["hits"]) and int(z["rows_seen"]) == frames
        assert np.array_equal(z["upper"], upper) and np.all(np.isneginf(z["lower"]))
        assert z["event_rows"].dtype == np.float32 and np.array_equal(z["event_rows"], db[bursts[:3]])
        assert mm.events_equal(d["maskEvents"], want["events"]) and d["maskEventsTotal"] == len(bursts)
        assert np.array_equal(d["maskHits"], want["hits"]) and d["maskRows"] == frames
        assert np.array_equal(d["maskEventRows"], db[bursts[:3]])
        assert re.search(r"^INFO:zero_span: mask rows \[%d\], events stored \[3\] / total \[%d\]" % (frames, len(bursts)), out, flags=re.M)
        for k in ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg", "fftHM"):
            assert np.array_equal(d[k], plain[k]), (batch, k)              # bit for bit
        assert d["fftHMIndex"] == plain["fftHMIndex"] == frames % 128
    # with the density on as well: both consume the same rows
    d, _ = run(["frameBatch", "8", "mask", "learn:%d:6:events=3" % learn, "density", "64:-120:0"])
    assert mm.events_equal(d["maskEvents"], want["events"]) and d["densityRows"] == frames
