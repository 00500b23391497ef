"""The pulse detector on the GPU against tests/pulse_model.py (checked on hand-worked cases on the CPU, in
tests/test_pulse_host.py).  Every comparison is np.array_equal, field by field: the arithmetic of include/ksa_pulse.h is
integer from q on.  Lengths sit on every edge of the window and of the tile T = kernel_info()['tile']: 0, 1, 2, W-1, W, W+1,
T-1, T, T+1, 3T+5, for W in 1, 2, 7, 64, 4096; every input format once and once from a pointer one sample into a 16-byte-aligned
allocation; no input exceeds 2^17 samples."""
import importlib
import re

import numpy as np
import pytest

import pulse_model as pm
from conftest import load_pkg

pytestmark = pytest.mark.gpu

FMTS = ("c64", "u8", "s8", "s16")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def X():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.pulse")


def sample_bytes(raw):
    return 8 if raw.dtype == np.complex64 else 2 * raw.dtype.itemsize


def to_dev(torch, raw, offset=0):
    """(tensor that owns the memory, device address of the samples): raw is complex64 [n] or an integer array [n][2]; `offset`
    samples into a 16-byte-aligned allocation."""
    raw = np.ascontiguousarray(raw)
    per = sample_bytes(raw)
    b = raw.view(np.uint8).reshape(-1)
    buf = torch.zeros(len(b) + per * offset + 16, dtype=torch.uint8, device="cuda")
    if len(b):
        buf[per * offset:per * offset + len(b)] = torch.from_numpy(b.copy())
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + per * offset


def events_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and all(np.array_equal(a[k], b[k]) for k in a.dtype.names)


def run_stream(torch, det, raw, pieces=None, offset=0, flush=True):
    """raw through process_dev in pieces (None: whole) with dense output; returns (S, events, total, active)."""
    n = len(raw)
    env = torch.full((max(n, 1) + 3,), -7, dtype=torch.int64, device="cuda")
    keep, ptr = to_dev(torch, raw, offset)
    per = sample_bytes(raw)
    at = 0
    for p in ([n] if pieces is None else pieces):
        det.process_dev(ptr + per * at if p else 0, p, env=env.data_ptr() + 8 * at if p else None)
        at += p
    assert at == n and det.state()["samples_in"] == n
    if flush:
        det.flush()
    ev, total, active = det.events()
    S = env.cpu().numpy()
    assert np.all(S[n:] == -7), "nothing is written past the samples of the call"
    return S[:n].copy(), ev, total, active


def bursty_s16(rng, n, period=300):
    """int16 [n][2]: weak noise with strong bursts of random lengths."""
    iq = rng.integers(-1000, 1001, (n, 2)).astype(np.int16)
    at = int(rng.integers(0, period))
    while at < n:
        ln = int(rng.integers(1, period))
        iq[at:at + ln] = rng.integers(-16000, 16001, (min(n, at + ln) - at, 2))
        at += ln + int(rng.integers(1, period))
    return iq


def check_against_model(got, raw, W, on, off, min_len=1, fmt="c64", capacity=None, **kw):
    S, ev, total, active = got
    wS, wev, _ = pm.detect(raw, W, on, off, min_len, fmt, **kw)
    assert np.array_equal(S, wS)
    assert total == len(wev) and active == int(wev["len"].sum())
    assert events_equal(ev, wev if capacity is None else wev[:capacity])
    return wev


# ------------------------------------------------------------------------------------------ lengths, windows, formats
@pytest.mark.parametrize("W", [1, 2, 7, 64, 4096])
def test_every_edge_of_the_window_and_of_the_tile(X, torch_cuda, W):
    det = X.PulseDetector(W=W, on_power=0.05, off_power=0.02, capacity=4096, max_in=1 << 17, fmt="s16")
    T = det.kernel_info()["tile"]
    assert det.thresholds() == pm.thresholds(0.05, 0.02, W)
    rng = np.random.default_rng(100 + W)
    seen = 0
    for n in sorted({0, 1, 2, W - 1, W, W + 1, T - 1, T, T + 1, 3 * T + 5}):
        raw = bursty_s16(rng, n)
        det.reset()
        wev = check_against_model(run_stream(torch_cuda, det, raw), raw, W, 0.05, 0.02, fmt="s16")
        seen += len(wev)
    assert seen > 3                                                  # W = 4096 sees a few long runs, the others dozens
    det.close()


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("fmt", FMTS)
def test_every_input_format_aligned_and_one_sample_in(X, torch_cuda, fmt, offset):
    rng = np.random.default_rng(7 + offset)
    s16 = bursty_s16(rng, 3 * 2048 + 5)
    if fmt == "c64":
        raw = ((s16[:, 0] + 1j * s16[:, 1]) / 32768.0 * 1.7).astype(np.complex64)
    elif fmt == "u8":
        raw = np.clip(s16 // 128 + 128, 0, 255).astype(np.uint8)
    elif fmt == "s8":
        raw = (s16 // 256).astype(np.int8)
    else:
        raw = s16
    kw = dict(u8_offset=127.4, u8_scale=127.6) if fmt == "u8" else {}
    det = X.PulseDetector(W=7, on_power=0.05, off_power=0.02, capacity=4096, max_in=1 << 14, fmt=fmt, **kw)
    wev = check_against_model(run_stream(torch_cuda, det, raw, offset=offset), raw, 7, 0.05, 0.02, fmt=fmt, **kw)
    assert len(wev) > 5
    # the host form gives the same
    det.reset()
    S = det.process(raw)
    det.flush()
    check_against_model((S,) + det.events(), raw, 7, 0.05, 0.02, fmt=fmt, **kw)
    det.close()


def test_saturation_counts_as_four(X, torch_cuda):
    x = np.zeros(40, dtype=np.complex64)
    x[10], x[11], x[20] = 3, 3j, 2                                   # |x|^2 = 9, 9 and exactly 4
    det = X.PulseDetector(W=1, on_power=4.0, off_power=4.0, max_in=64)
    S, ev, total, active = run_stream(torch_cuda, det, x)
    assert S[10] == S[11] == S[20] == 4 << 30 and S.sum() == 3 * (4 << 30)
    check_against_model((S, ev, total, active), x, 1, 4.0, 4.0)
    assert [(int(e["start"]), int(e["len"]), int(e["energy"])) for e in ev] == [(10, 2, 8 << 30), (20, 1, 4 << 30)]
    # x[11] conj(x[10]) = 9j: clamped to 4
    assert (int(ev[0]["dre"]), int(ev[0]["dim"])) == (0, 4 << 30)
    det.close()


# ------------------------------------------------------------------------------------------ planted runs
def planted(T):
    """complex64 signal and the runs planted in it, W = 4, on 0.1, off 0.05: amplitude 0.5 is on, 0.27 holds, 0.01 is off."""
    lo, mid, hi = 0.01, 0.27, 0.5
    n = 16 * T + 77
    a = np.full(n, lo)
    a[0:50] = hi
    a[0:2] = 1.5                                                     # q[0] alone reaches thr_on at W = 4 and 16: a run starts at sample 0
    a[T - 20:T + 30] = hi                                            # crosses one tile border
    a[2 * T - 5:5 * T + 9] = hi                                      # covers three whole tiles
    a[6 * T + 100:6 * T + 200] = hi                                  # set ...
    a[6 * T + 200:8 * T + 300] = mid                                 # ... and a HOLD stretch over a whole tile keeps it
    a[9 * T + 10:11 * T + 500] = mid                                 # a HOLD stretch over a whole tile with the state clear
    a[11 * T + 500:11 * T + 600] = hi
    a[13 * T:14 * T] = hi                                            # exactly one tile
    a[n - 300:] = hi                                                 # still active at the end
    ph = np.exp(2j * np.pi * 0.05 * np.arange(n))
    return (a * ph).astype(np.complex64)


def test_planted_runs_across_tiles_and_hold_stretches(X, torch_cuda):
    det = X.PulseDetector(W=4, on_power=0.1, off_power=0.05, capacity=64, max_in=1 << 17)
    T = det.kernel_info()["tile"]
    x = planted(T)
    got = run_stream(torch_cuda, det, x)
    wev = check_against_model(got, x, 4, 0.1, 0.05)
    starts, lens = list(wev["start"]), list(wev["len"])
    assert starts[0] == 0 and len(wev) == 7
    assert any(s < T < s + l for s, l in zip(starts, lens))                                 # crosses a border
    assert any(s < 2 * T and s + l > 5 * T for s, l in zip(starts, lens))                   # three whole tiles inside
    assert any(6 * T < s < 7 * T and s + l > 8 * T + 200 for s, l in zip(starts, lens))     # HOLD kept it set over tile 7
    assert not any(9 * T <= s < 11 * T + 400 for s in starts)                               # HOLD with the state clear
    assert list(wev["flags"]) == [0] * 6 + [X.FLAG_OPEN_END] and starts[-1] + lens[-1] == len(x)
    assert det.state() == {"samples_in": len(x), "open": False, "open_start": -1}
    # without the flush the last run stays open and is not listed
    det.reset()
    S, ev, total, active = run_stream(torch_cuda, det, x, flush=False)
    assert total == 6 and events_equal(ev, wev[:6])
    assert det.state() == {"samples_in": len(x), "open": True, "open_start": int(starts[-1])}
    # the block form flags it too
    det.reset()
    keep, ptr = to_dev(torch_cuda, x)
    det.blocks_dev(ptr, 1, len(x))
    ev, total, active = det.events()
    want = wev.copy()
    want["block"] = 0
    assert events_equal(ev, want) and total == 7 and active == int(wev["len"].sum())
    assert det.state() == {"samples_in": 0, "open": False, "open_start": -1}
    det.close()


def test_runs_of_exactly_min_len_and_one_less(X, torch_cuda):
    det = X.PulseDetector(W=1, on_power=0.25, off_power=0.25, min_len=10, capacity=64, max_in=1 << 14)
    T = det.kernel_info()["tile"]
    x = np.zeros(3 * T, dtype=np.complex64)
    runs = [(5, 10), (40, 9), (T - 4, 10), (T + 100, 9), (2 * T - 9, 9), (2 * T + 7, 11), (3 * T - 10, 10), (300, 1)]
    for s, l in runs:
        x[s:s + l] = 0.5                                             # S exactly thr_on
    got = run_stream(torch_cuda, det, x)
    wev = check_against_model(got, x, 1, 0.25, 0.25, min_len=10)
    assert sorted(zip(wev["start"], wev["len"])) == sorted((s, l) for s, l in runs if l >= 10)
    assert got[3] == 10 + 10 + 11 + 10                               # the dropped runs are counted nowhere
    assert wev[-1]["flags"] == X.FLAG_OPEN_END and list(wev["flags"][:-1]) == [0, 0, 0]
    det.close()


def test_random_int16_noise_with_bursts(X, torch_cuda):
    rng = np.random.default_rng(31)
    raw = bursty_s16(rng, 1 << 17, period=900)
    det = X.PulseDetector(W=16, on_power=0.06, off_power=0.03, min_len=3, capacity=1 << 12, max_in=1 << 17, fmt="s16")
    assert det.thresholds() == pm.thresholds(0.06, 0.03, 16)
    wev = check_against_model(run_stream(torch_cuda, det, raw), raw, 16, 0.06, 0.03, min_len=3, fmt="s16")
    assert len(wev) > 100
    det.close()


def test_capacity_keeps_the_first_and_clear_leaves_the_stream_alone(X, torch_cuda):
    rng = np.random.default_rng(5)
    raw = bursty_s16(rng, 3 * 2048 + 5)
    wS, wev, act = pm.detect(raw, 7, 0.05, 0.02, fmt="s16")
    assert len(wev) > 8
    det = X.PulseDetector(W=7, on_power=0.05, off_power=0.02, capacity=3, max_in=1 << 14, fmt="s16")
    check_against_model(run_stream(torch_cuda, det, raw), raw, 7, 0.05, 0.02, fmt="s16", capacity=3)
    # cut inside a run, clear between the calls: the second call's records are the model's from there on, the first of them
    # with its start before the cut
    mid = wev[len(wev) // 2]
    cut = int(mid["start"] + mid["len"] // 2) if mid["len"] > 1 else int(mid["start"]) + 1
    assert act[cut - 1]
    big = X.PulseDetector(W=7, on_power=0.05, off_power=0.02, capacity=4096, max_in=1 << 14, fmt="s16")
    keep, ptr = to_dev(torch_cuda, raw)
    big.process_dev(ptr, cut)
    before = big.state()
    first, total, _ = big.events()
    big.clear_events()
    assert big.state() == before and before["open"] and before["open_start"] == int(mid["start"])
    assert big.events()[1:] == (0, 0) and len(big.events()[0]) == 0
    big.process_dev(ptr + 4 * cut, len(raw) - cut)
    big.flush()
    second, total2, active2 = big.events()
    assert events_equal(np.concatenate([first, second]), wev) and total + total2 == len(wev)
    assert int(second[0]["start"]) < cut and active2 == int(second["len"].sum())
    det.close()
    big.close()


# ------------------------------------------------------------------------------------------ cutting
def test_the_cut_of_a_stream_is_invisible(X, torch_cuda):
    W = 16
    det = X.PulseDetector(W=W, on_power=0.1, off_power=0.05, capacity=256, max_in=1 << 17)
    T = det.kernel_info()["tile"]
    x = planted(T)[:9 * T]
    n = len(x)
    whole = run_stream(torch_cuda, det, x)
    wev = check_against_model(whole, x, W, 0.1, 0.05)
    in_run = int(wev[2]["start"] + wev[2]["len"] // 2)               # inside the run over three tiles
    in_hold = 7 * T + 11                                             # inside the HOLD stretch
    for pieces in ([1, n - 1], [0, 5, 0, n - 5], [in_run, n - in_run], [in_hold, n - in_hold], [in_run, in_hold - in_run, 1, n - in_hold - 1],
                   [T, T, T, n - 3 * T], [n - 1, 1]):
        det.reset()
        S, ev, total, active = run_stream(torch_cuda, det, x, pieces=pieces)
        assert np.array_equal(S, whole[0]) and events_equal(ev, whole[1]) and (total, active) == whole[2:], pieces
    # every piece of length 1
    m = 2 * W + 9
    y = x[30:30 + m]                                                 # the first run's end and what follows it
    assert len(y) == m
    det.reset()
    one = run_stream(torch_cuda, det, y)
    check_against_model(one, y, W, 0.1, 0.05)
    assert one[2] >= 1
    det.reset()
    S, ev, total, active = run_stream(torch_cuda, det, y, pieces=[1] * m)
    assert np.array_equal(S, one[0]) and events_equal(ev, one[1]) and (total, active) == one[2:]
    det.close()


def test_overlapping_blocks_equal_fresh_streams_with_flush(X, torch_cuda):
    rng = np.random.default_rng(77)
    nb, stride, blen = 5, 1500, 2 * 2048 + 300
    raw = bursty_s16(rng, (nb - 1) * stride + blen)
    det = X.PulseDetector(W=64, on_power=0.05, off_power=0.02, min_len=2, capacity=4096, max_in=nb * blen, fmt="s16")
    keep, ptr = to_dev(torch_cuda, raw)
    out_stride = blen + 7
    env = torch_cuda.full((nb * out_stride,), -7, dtype=torch_cuda.int64, device="cuda")
    det.blocks_dev(ptr, nb, blen, block_stride=stride, env=env.data_ptr(), out_stride=out_stride)
    ev, total, active = det.events()
    S = env.cpu().numpy().reshape(nb, out_stride)
    assert np.all(S[:, blen:] == -7)
    assert det.state() == {"samples_in": 0, "open": False, "open_start": -1}
    parts = []
    one = X.PulseDetector(W=64, on_power=0.05, off_power=0.02, min_len=2, capacity=4096, max_in=blen, fmt="s16")
    for b in range(nb):
        blk = raw[b * stride:b * stride + blen]
        one.reset()
        sS, sev, _, _ = run_stream(torch_cuda, one, blk)
        wS, wev, _ = pm.detect(blk, 64, 0.05, 0.02, 2, "s16", block=b)
        assert np.array_equal(S[b, :blen], sS) and np.array_equal(sS, wS)
        sev["block"] = b
        assert events_equal(sev, wev)
        parts.append(wev)
    want = np.concatenate(parts)
    assert events_equal(ev, want) and total == len(want) and active == int(want["len"].sum())
    assert np.any(want["flags"] == X.FLAG_OPEN_END) and len(want) > 10
    # blocks append behind what the list already holds
    det.blocks_dev(ptr, 2, blen, block_stride=stride)
    ev2, total2, _ = det.events()
    assert total2 == len(want) + len(parts[0]) + len(parts[1]) and events_equal(ev2[len(want):], np.concatenate(parts[:2]))
    det.close()
    one.close()


# ------------------------------------------------------------------------------------------ parameters, state, refusals
def test_set_params_reset_and_refusal_after_flush(X, torch_cuda):
    rng = np.random.default_rng(11)
    raw = bursty_s16(rng, 5000)
    det = X.PulseDetector(W=7, on_power=0.05, off_power=0.02, capacity=4096, max_in=1 << 14, fmt="s16")
    keep, ptr = to_dev(torch_cuda, raw)
    det.process_dev(ptr, 2000)
    det.set_params(0.2, 0.1)                                         # holds from the next call
    assert det.thresholds() == pm.thresholds(0.2, 0.1, 7)
    with pytest.raises(X.KsaError, match="off_power 0.5"):
        det.set_params(0.2, 0.5)
    assert det.thresholds() == pm.thresholds(0.2, 0.1, 7) and (det.on_power, det.off_power) == (0.2, 0.1)
    det.process_dev(ptr + 4 * 2000, 3000)
    det.flush()
    ev, total, active = det.events()
    # the model with the levels changed at sample 2000
    xr, xi = pm.unpack(raw, "s16")
    q, dre, dim = pm.quantities(xr, xi)
    S = pm.envelope(q, 7)
    a_on, a_off = pm.thresholds(0.05, 0.02, 7)
    b_on, b_off = pm.thresholds(0.2, 0.1, 7)
    act, state = np.zeros(len(S), dtype=bool), False
    for n, s in enumerate(S.tolist()):
        on, off = (a_on, a_off) if n < 2000 else (b_on, b_off)
        state = True if s >= on else False if s < off else state
        act[n] = state
    want = pm.runs_of(q, dre, dim, S, act, 1)
    assert events_equal(ev, want) and total == len(want) and len(want) > 3
    for call in (lambda: det.process_dev(ptr, 10), lambda: det.process(raw[:10]), det.flush):
        with pytest.raises(X.KsaError, match="the stream was flushed; kpl_reset starts a new stream"):
            call()
    det.blocks_dev(ptr, 1, 100)                                      # the block form is not a stream call
    det.reset()
    assert det.state() == {"samples_in": 0, "open": False, "open_start": -1} and det.events()[1:] == (0, 0)
    check_against_model(run_stream(torch_cuda, det, raw), raw, 7, 0.2, 0.1, fmt="s16")
    det.close()


def test_refused_calls_leave_the_object_as_it_was(X, torch_cuda):
    rng = np.random.default_rng(12)
    raw = bursty_s16(rng, 4000)
    det = X.PulseDetector(W=7, on_power=0.05, off_power=0.02, capacity=4096, max_in=3000, fmt="s16")
    keep, ptr = to_dev(torch_cuda, raw)
    env = torch_cuda.zeros(4000, dtype=torch_cuda.int64, device="cuda")
    det.process_dev(ptr, 1000)
    before, ev0 = det.state(), det.events()
    for call, text in ((lambda: det.process_dev(ptr, -1), "n_in -1 must be >= 0"),
                       (lambda: det.process_dev(ptr, 3001), "n_in 3001 exceeds max_in 3000"),
                       (lambda: det.process_dev(None, 5), "null input pointer"),
                       (lambda: det.process_dev(ptr + 2, 5), "input pointer is not aligned to the 4 bytes of a sample"),
                       (lambda: det.blocks_dev(ptr, -1, 10), "nblocks -1 must be >= 0"),
                       (lambda: det.blocks_dev(ptr, 1, -10, block_stride=10), "block_len -10 must be >= 0"),
                       (lambda: det.blocks_dev(ptr, 1, 10, block_stride=-1), "block_stride -1 must be >= 0"),
                       (lambda: det.blocks_dev(ptr, 4, 1000), "4 blocks of 1000 samples exceed max_in 3000"),
                       (lambda: det.blocks_dev(ptr, 1, 3001), "1 blocks of 3001 samples exceed max_in 3000"),
                       (lambda: det.blocks_dev(None, 1, 10), "null input pointer"),
                       (lambda: det.blocks_dev(ptr + 1, 1, 10), "input pointer is not aligned"),
                       (lambda: det.blocks_dev(ptr, 2, 100, env=env.data_ptr(), out_stride=99),
                        "out_stride 99 is shorter than the 100 samples of a block")):
        with pytest.raises(X.KsaError) as e:
            call()
        assert text in str(e.value), (text, str(e.value))
        assert det.state() == before
    now = det.events()
    assert events_equal(now[0], ev0[0]) and now[1:] == ev0[1:]
    det.process_dev(0, 0)                                            # n_in = 0 is a no-op
    det.blocks_dev(0, 0, 10)
    assert det.state() == before
    det.process_dev(ptr + 4 * 1000, 3000)
    det.flush()
    check_against_model((pm.detect(raw, 7, 0.05, 0.02, 1, "s16")[0],) + det.events(), raw, 7, 0.05, 0.02, fmt="s16")
    info = det.kernel_info()
    assert info["threads"] == 256 and info["tile"] == 2048 and info["lds_bytes"] >= (2048 + 7) * 8 and info["grid"] >= 1
    det.close()


# ------------------------------------------------------------------------------------------ command line
def test_cli_pulses_reports_and_saves(X, torch_cuda, tmp_path, capsys):
    Kmod = importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")
    frames, rate, W = 4, 2048000, 16
    rng = np.random.default_rng(2025)
    save, capture = tmp_path / "out.npz", tmp_path / "capture.s16"
    common = ["zeroSpan", "fftSize", "1024", "samplingRate", str(rate), "iqFormat", "s16", "bPltLevels", "false", "bPltHeatMap", "false",
              "prgLoopCnt", str(frames), "frameBatch", "2"]
    full = Kmod.handle_args({}, common)["fullSize"]
    want_read = int(2 ** np.ceil(np.log2(full)))                     # what one block consumes of the capture
    settle = 16 * 1024
    x = (rng.standard_normal((frames, want_read)) + 1j * rng.standard_normal((frames, want_read))) * 0.004
    f0 = 50000.0
    planted_at = [(0, 100, 400), (1, full - 700, 300), (3, 900, 1000)]
    for b, s, ln in planted_at:
        x[b, s:s + ln] += 0.5 * np.exp(2j * np.pi * f0 / rate * np.arange(ln))
    iq = np.zeros((settle + frames * want_read, 2), dtype=np.int16)
    flat = x.reshape(-1)
    iq[settle:, 0], iq[settle:, 1] = np.rint(flat.real * 32768 * 0.5), np.rint(flat.imag * 32768 * 0.5)
    iq.tofile(capture)
    Kmod.sdr_curscan = Kmod._gpu_curscan
    capsys.readouterr()
    d = Kmod.main(common + ["source", "file:%s" % capture, "pulses", "-20:-26:%d:8" % W, "pulsesSave", str(save)])
    out = capsys.readouterr().out
    on, off = X.db_to_power(-20), X.db_to_power(-26)
    parts = []
    for b in range(frames):
        blk = iq[settle + b * want_read:settle + b * want_read + full]
        parts.append(pm.detect(blk, W, on, off, 8, "s16", block=b)[1])
    want = np.concatenate(parts)
    ev = d["pulseEvents"]
    assert len(want) == 3 and events_equal(ev, want) and d["pulseTotal"] == 3 and d["pulseActive"] == int(want["len"].sum())
    for e, (b, s, ln) in zip(ev, planted_at):
        assert int(e["block"]) == b and abs(int(e["start"]) - s) <= W and abs(int(e["len"]) - ln) <= 2 * W
    thr_on, thr_off = pm.thresholds(on, off, W)
    assert re.search(r"^INFO:zero_span: pulses blocks \[4\], W \[16\], thr_on \[%d\] thr_off \[%d\], pulses stored \[3\] / total \[3\], "
                     r"active samples \[%d\]" % (thr_on, thr_off, d["pulseActive"]), out, flags=re.M), out[-600:]
    z = np.load(save)
    assert sorted(z.files) == sorted(["events", "pulses_total", "active_total", "rel", "on_db", "off_db", "W", "min_len", "capacity",
                                      "thr_on", "thr_off", "sampling_rate", "block_len", "toa_s", "width_s", "mean_dbfs", "peak_dbfs",
                                      "freq_hz"])
    assert events_equal(z["events"], want) and int(z["pulses_total"]) == 3 and int(z["active_total"]) == d["pulseActive"]
    for k, v in pm.describe(want, W, rate, full).items():
        assert np.array_equal(z[k], v), k
    assert np.all(np.abs(z["freq_hz"] - f0) <= rate / (2 * np.pi * want["len"])), z["freq_hz"]
    assert np.all(np.abs(z["mean_dbfs"] - 10 * np.log10(0.0625)) < 0.5)
    assert (int(z["W"]), int(z["min_len"]), int(z["capacity"]), int(z["block_len"]), bool(z["rel"])) == (W, 8, 1024, full, False)
    assert (int(z["thr_on"]), int(z["thr_off"]), float(z["on_db"]), float(z["off_db"])) == (thr_on, thr_off, -20.0, -26.0)
    # rel: the same bursts, levels above the median envelope of the first block
    d = Kmod.main(common + ["source", "file:%s" % capture, "pulses", "rel:20:14:%d:8" % W])
    out = capsys.readouterr().out
    S0 = pm.detect(iq[settle:settle + full], W, 1.0, 1.0, 1, "s16")[0]
    base = float(np.median(S0)) / W / pm.UNIT
    r_on, r_off = base * 10.0 ** 2.0, base * 10.0 ** 1.4
    parts = [pm.detect(iq[settle + b * want_read:settle + b * want_read + full], W, r_on, r_off, 8, "s16", block=b)[1] for b in range(frames)]
    want = np.concatenate(parts)
    assert len(want) == 3 and events_equal(d["pulseEvents"], want) and d["pulseTotal"] == 3
    assert "thr_on [%d] thr_off [%d]" % pm.thresholds(r_on, r_off, W) in out
