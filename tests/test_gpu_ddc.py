"""The digital down-converter on the GPU against tests/ddc_model.py (whose float32 emulation is checked against the bound on
the CPU, in tests/test_ddc_host.py).  Shapes (D, T) are the smallest at which the filter takes
each of its paths: one tap, odd and even D, every register blocking of the tile form (PLANS below names each shape's: four outputs
per thread, two -- (8, 64) and, with fewer taps than the decimation, (8, 3) --, one), the large-span tile form and the reduce
form with several chunks; every test asserts the plan it expects from kernel_info; output counts sit either side of a workgroup's tile (kernel_info's tile_out), which also moves the
16-byte loads of a tile over every alignment.  Impulses and integers are compared exactly, floats against the bound written
down in ddc_model.bound."""
import importlib

import numpy as np
import pytest

import ddc_model as dm
from conftest import load_pkg

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 33), (2, 16), (3, 11), (4, 32), (5, 35), (8, 64), (8, 3), (16, 128), (64, 1024), (1024, 16384)]
# (D, T) -> (tile_out, form) of kernel_info: 256 threads x 4, 2 or 1 outputs (FORM_TILE = 0); 8 outputs in the reduce form (1).
# Two outputs per thread where 511 D + T <= 7680 < 1023 D + T, one up to 255 D + T <= 17408, the reduce form beyond.
PLANS = {(1, 1): (1024, 0), (1, 33): (1024, 0), (2, 16): (1024, 0), (3, 11): (1024, 0), (4, 32): (1024, 0), (5, 35): (1024, 0),
         (8, 64): (512, 0), (8, 3): (512, 0), (16, 128): (256, 0), (64, 1024): (256, 0), (1024, 16384): (8, 1)}
INT_SHAPES = [s for s in SHAPES if s[1] <= 64]
FMTS = (dm.FMT_C64, dm.FMT_U8, dm.FMT_S8, dm.FMT_S16)
INC = round(0.1234567 * 2 ** 64)
WORST = {}                                   # (D, T) -> worst error / bound of the float test, printed at the end


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def X():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.ddc")


def counts_for(dc, shape):
    info = dc.kernel_info()
    assert (info["tile_out"], info["form"]) == PLANS[shape], (shape, info)
    t = info["tile_out"]
    return [1, 3 * t + 7] if shape == SHAPES[-1] else sorted({1, max(1, t - 1), t, t + 1, 3 * t + 7})


def lowpass(X, D, T):
    """ddc_lowpass where T is a whole number of phases, else the same formula at that T."""
    if T % D == 0:
        return X.ddc_lowpass(D, T // D)
    t = np.arange(T, dtype=np.float64) - (T - 1) / 2
    h = np.sinc(0.8 * t / D) * np.hamming(T)
    return (h / h.sum()).astype(np.float32)


def random_raw(rng, fmt, n):
    """Unit-scale random samples in the raw form of fmt."""
    if fmt == dm.FMT_C64:
        return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)
    info = {dm.FMT_U8: (0, 256, np.uint8), dm.FMT_S8: (-128, 128, np.int8), dm.FMT_S16: (-32768, 32768, np.int16)}[fmt]
    return rng.integers(info[0], info[1], 2 * n).astype(info[2])


def to_dev(torch, raw):
    if raw.dtype == np.complex64:
        return torch.view_as_real(torch.from_numpy(raw)).cuda()
    return torch.from_numpy(raw).cuda()


def run_stream(torch, dc, raw, n_in, first=0):
    """Samples [first, first + n_in) of raw through process_dev into a caller's buffer; complex64 on the host."""
    per = 1 if raw.dtype == np.complex64 else 2
    want = dc.out_count(n_in)
    out = torch.zeros(max(want, 1), dtype=torch.complex64, device="cuda")
    got = dc.process_dev(to_dev(torch, raw[per * first:per * (first + n_in)]) if n_in else 0, n_in, out=out, out_capacity=want)
    assert got == want
    dc.synchronize()
    return out[:got].cpu().numpy()


def own_buffer(torch, dc, n):
    dc.synchronize()
    return torch.as_tensor(dc.out, device="cuda")[:n].cpu().numpy()


# ------------------------------------------------------------------------------------------ 1. impulse, exact
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_impulse_places_every_tap_exactly(X, torch_cuda, shape):
    D, T = shape
    rng = np.random.default_rng(D * 100003 + T)
    taps = rng.uniform(-1, 1, T).astype(np.float32)
    dc = X.DownConverter(dm.FMT_C64, D, taps, phase_inc=0, max_in=1 << 18)
    t = dc.kernel_info()["tile_out"]
    for count in counts_for(dc, shape):
        n_in = D * (count - 1) + 1
        spots = {0, 1, D - 1, D, T - 1}
        for m0 in range(t, count, t):                  # either side of each later tile's oldest and newest first input
            for s in (m0 * D - (T - 1), m0 * D):
                spots.update((s - 1, s, s + 1))
        for p in sorted(s for s in spots if 0 <= s < n_in):
            for value in (1.0, 1j):
                x = np.zeros(n_in, dtype=np.complex64)
                x[p] = value
                dc.reset()
                y = dc.process(x)
                k = np.arange(count) * D - p
                want = np.where((k >= 0) & (k < T), taps[np.clip(k, 0, T - 1)], np.float32(0)).astype(np.complex64) * np.complex64(value)
                assert y.shape == (count,) and np.array_equal(y, want), (shape, count, p, value)
    dc.close()


# ------------------------------------------------------------------------------------------ 2. integers, exact
def int_raw(rng, fmt, n, amp):
    """Raw samples whose integer values stay within +-amp (uint8: around 128; complex64: k / 2^15)."""
    b = rng.integers(-amp, amp + 1, 2 * n)
    if fmt == dm.FMT_C64:
        return ((b[0::2] + 1j * b[1::2]) / 32768.0).astype(np.complex64)
    if fmt == dm.FMT_U8:
        return (b + 128).astype(np.uint8)
    return b.astype(np.int8 if fmt == dm.FMT_S8 else np.int16)


@pytest.mark.parametrize("shape", INT_SHAPES, ids=str)
def test_integers_are_exact_in_every_format(X, torch_cuda, shape):
    D, T = shape
    rng = np.random.default_rng(D * 7919 + T)
    taps = rng.integers(-8, 9, T)
    taps[0], taps[-1] = 8, -7                          # the outermost taps are there
    budget = 2 ** 23 // int(np.abs(taps).sum())        # sum|h| max|b| <= 2^23: every partial sum is a float32 value
    for fmt in FMTS:
        amp = min(budget, {dm.FMT_C64: 32767, dm.FMT_U8: 127, dm.FMT_S8: 127, dm.FMT_S16: 32767}[fmt])
        kw = dict(u8_offset=128.0, u8_scale=128.0) if fmt == dm.FMT_U8 else {}
        for inc in (0, 2 ** 62, 2 ** 63, 3 * 2 ** 62):
            dc = X.DownConverter(fmt, D, taps.astype(np.float32), phase_inc=inc, max_in=1 << 18, **kw)
            for count in counts_for(dc, shape):
                n_in = D * (count - 1) + 1
                raw = int_raw(rng, fmt, n_in, amp)
                iq, scale = dm.to_int(raw, fmt)
                want = dm.int_stream(iq, scale, taps, D, dm.phases(n_in, inc))
                dc.reset()
                assert np.array_equal(run_stream(torch_cuda, dc, raw, n_in), want), (shape, fmt, inc, count, "stream")
                # the block form: three overlapping blocks of `count` outputs each
                block_len = D * (count - 1) + T
                stride = max(1, block_len // 2)
                braw = int_raw(rng, fmt, 2 * stride + block_len, amp)
                biq, scale = dm.to_int(braw, fmt)
                wantb = dm.int_blocks(biq, scale, taps, D, inc, 3, block_len, [0, stride, 2 * stride])
                assert dc.blocks_dev(to_dev(torch_cuda, braw), 3, block_len, block_stride=stride) == count
                got = own_buffer(torch_cuda, dc, 3 * count).reshape(3, count)
                assert np.array_equal(got, wantb), (shape, fmt, inc, count, "blocks")
                if count == 1 or inc:
                    continue
                # the premise, on the CPU: float32 sums forwards and backwards both give the integer model's values
                v = (iq[:, 0] + 1j * iq[:, 1]) / scale
                for backwards in (False, True):
                    assert np.array_equal(dm.f32_fir(v, taps, D, 0, count, backwards), want)
            dc.close()


# ------------------------------------------------------------------------------------------ 3. floats, bounded
def check_bound(got, want, taps, max_abs, shape, what):
    limit = dm.bound(taps, max_abs)
    worst = float(np.max(np.abs(got.astype(np.complex128) - want))) / limit if len(got) else 0.0
    WORST[shape] = max(WORST.get(shape, 0.0), worst)
    print("ddc float test %s %s: worst error / bound = %.4f" % (shape, what, worst))
    assert got.shape == want.shape and worst <= 1.0, (shape, what, worst)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_floats_stay_inside_the_bound(X, torch_cuda, shape):
    D, T = shape
    rng = np.random.default_rng(D * 31337 + T)
    taps = lowpass(X, D, T)
    for fmt in FMTS:
        dc = X.DownConverter(fmt, D, taps, phase_inc=INC, max_in=1 << 18)
        for count in counts_for(dc, shape):
            n_in = D * (count - 1) + 1
            raw = random_raw(rng, fmt, n_in)
            x = dm.unpack(raw, fmt)
            phi = dm.phases(n_in, INC)
            want = dm.fir_at(x * dm.rotor(phi), taps, D, 0, count)
            dc.reset()
            check_bound(run_stream(torch_cuda, dc, raw, n_in), want, taps, np.abs(x).max(), shape, "fmt %d count %d stream" % (fmt, count))
        count = counts_for(dc, shape)[-2]
        block_len = D * (count - 1) + T
        raw = random_raw(rng, fmt, 2 * block_len)
        x = dm.unpack(raw, fmt).reshape(2, block_len)
        want = np.array([dm.fir_at(row * dm.rotor(dm.phases(block_len, INC)), taps, D, T - 1, count) for row in x])
        assert dc.blocks_dev(to_dev(torch_cuda, raw), 2, block_len) == count
        check_bound(own_buffer(torch_cuda, dc, 2 * count).reshape(2, count), want, taps, np.abs(x).max(), shape, "fmt %d blocks" % fmt)
        dc.close()


def test_report_the_worst_ratio():
    print("ddc float test: worst error / bound per shape:", {k: round(v, 4) for k, v in WORST.items()})
    assert all(v <= 1.0 for v in WORST.values())


# ------------------------------------------------------------------------------------------ 4. cuts
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_the_cut_of_the_stream_does_not_show(X, torch_cuda, shape):
    D, T = shape
    rng = np.random.default_rng(D * 271 + T)
    taps = lowpass(X, D, T)
    for fmt in (dm.FMT_C64, dm.FMT_U8):
        dc = X.DownConverter(fmt, D, taps, phase_inc=INC, max_in=1 << 18)
        counts_for(dc, shape)                              # (asserts the plan)
        t = dc.kernel_info()["tile_out"]
        cuts = [1, D - 1, D, max(T - 2, 0), T - 1, T, 0]
        cuts.append(D * (2 * t + 5) + 3)
        n = sum(cuts)
        raw = random_raw(rng, fmt, n)
        whole = run_stream(torch_cuda, dc, raw, n)
        assert dc.state() == {"samples_in": n, "samples_out": len(whole), "phase": n * INC % 2 ** 64}
        dc.reset()
        assert dc.state() == {"samples_in": 0, "samples_out": 0, "phase": 0}
        parts, at = [], 0
        for c in cuts:
            assert dc.out_count(c) == dm.out_count(at, c, D)
            parts.append(run_stream(torch_cuda, dc, raw, c, first=at))
            assert len(parts[-1]) == dm.out_count(at, c, D)
            at += c
        pieces = np.concatenate(parts)
        assert np.array_equal(pieces.view(np.uint32), whole.view(np.uint32)), (shape, fmt)     # bit for bit
        # a retune in the middle follows the model's piecewise phase, and cutting there changes nothing either
        half, inc2 = n // 2 + 1, 2 ** 64 - INC // 3
        phi = dm.piecewise_phases([(half, INC), (n - half, inc2)])
        x = dm.unpack(raw, fmt)
        want = dm.fir_at(x * dm.rotor(phi), taps, D, 0, len(whole))
        dc.reset()
        a = run_stream(torch_cuda, dc, raw, half)
        dc.retune(phase_inc=inc2)
        b = run_stream(torch_cuda, dc, raw, n - half, first=half)
        assert dc.state()["phase"] == (half * INC + (n - half) * inc2) % 2 ** 64
        check_bound(np.concatenate([a, b]), want, taps, np.abs(x).max(), shape, "fmt %d retuned" % fmt)
        # reset restores the fresh result
        dc.retune(phase_inc=INC)
        dc.reset()
        again = run_stream(torch_cuda, dc, raw, n)
        assert np.array_equal(again.view(np.uint32), whole.view(np.uint32))
        dc.close()


# ------------------------------------------------------------------------------------------ 5. blocks
@pytest.mark.parametrize("shape", [(3, 11), (16, 128), (1024, 16384)], ids=str)
def test_blocks_at_every_stride_from_device_and_pinned_memory(ksa, X, torch_cuda, shape):
    torch = torch_cuda
    D, T = shape
    rng = np.random.default_rng(D * 977 + T)
    taps = lowpass(X, D, T)
    dc = X.DownConverter(dm.FMT_S16, D, taps, phase_inc=INC, max_in=1 << 22)
    t = dc.kernel_info()["tile_out"]
    M = t + 1 if D < 1024 else 2
    block_len = D * (M - 1) + T + (D - 1)              # the last D - 1 samples yield no further output
    assert dc.block_out_count(block_len) == M
    w = dm.rotor(dm.phases(block_len, INC))
    dc.process(random_raw(rng, dm.FMT_S16, 3 * D + 1))  # a stream is under way: the block form must not touch it
    state = dc.state()
    for nblocks in (1, 3, 130):
        for stride in (block_len, block_len + 5, block_len - min(block_len - 1, 2 * D + 1)):
            n = stride * (nblocks - 1) + block_len
            raw = random_raw(rng, dm.FMT_S16, n)
            x = dm.unpack(raw, dm.FMT_S16)
            want = np.array([dm.fir_at(x[b * stride:b * stride + block_len] * w, taps, D, T - 1, M) for b in range(nblocks)])
            assert dc.blocks_dev(to_dev(torch, raw), nblocks, block_len, block_stride=stride) == M
            own = own_buffer(torch, dc, nblocks * M).reshape(nblocks, M)
            check_bound(own, want, taps, np.abs(x).max(), shape, "blocks %d stride %d" % (nblocks, stride))
            # a caller's buffer at a wider stride, the input in page-locked memory: the same bits, nothing outside the rows
            pin = ksa.PinnedBuffer((2 * n,), np.int16)
            pin.array[:] = raw
            out = torch.full((nblocks, M + 3), 7 + 7j, dtype=torch.complex64, device="cuda")
            dc.blocks_dev(pin.array, nblocks, block_len, block_stride=stride, out=out, out_stride=M + 3)
            dc.synchronize()
            got = out.cpu().numpy()
            pin.close()
            assert np.array_equal(got[:, :M].view(np.uint32), own.view(np.uint32)) and np.all(got[:, M:] == 7 + 7j)
    assert dc.state() == state
    tail = random_raw(rng, dm.FMT_S16, 2 * D)
    fresh = X.DownConverter(dm.FMT_S16, D, taps, phase_inc=INC, max_in=1 << 22)
    rng2 = np.random.default_rng(D * 977 + T)
    fresh.process(random_raw(rng2, dm.FMT_S16, 3 * D + 1))
    assert np.array_equal(dc.process(tail).view(np.uint32), fresh.process(tail).view(np.uint32))   # the history too
    fresh.close()
    with pytest.raises(X.KsaError, match="shorter than the"):
        dc.blocks_dev(0, 0, T - 1)
    dc.close()


# ------------------------------------------------------------------------------------------ 6. into the engine
def test_zoomed_block_goes_into_the_engine(ksa, X, torch_cuda):
    import ksa_oracle as orc
    torch = torch_cuda
    D, n, full = 16, 1024, 2048
    taps = X.ddc_lowpass(D, 8)
    T = len(taps)
    block_len = D * (full - 1) + T
    f0 = 0.2                                           # the zoom's centre, cycles per input sample
    bin_in_span = 37                                   # delta: the tone sits 37 zoomed bins above the centre
    tone = f0 + bin_in_span / (n * D)
    tt = np.arange(block_len)
    x = (0.5 * np.exp(2j * np.pi * tone * tt) + 0.4 * np.exp(2j * np.pi * (f0 + 0.17) * tt)).astype(np.complex64)   # one inside, one outside
    inc = X.phase_inc_for(f0, 1.0)
    dc = X.DownConverter(dm.FMT_C64, D, taps, phase_inc=inc, max_in=block_len)
    assert dc.blocks_dev(to_dev(torch, x), 1, block_len) == full
    win = orc.window_table("hanning", n)
    eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=0.5, window="hanning", max_frames=1)
    out = torch.zeros(n, dtype=torch.float32, device="cuda")
    eng.curscan_dev(dc.out_ptr, ksa.FMT_C64, 1, out, ksa.OUT_LINEAR)
    eng.synchronize()
    got = out.cpu().numpy().astype(np.float64)
    y = dm.blocks(x.astype(np.complex128)[None, :], taps, D, inc)[0]
    assert y.shape == (full,)
    want = orc.curscan(y.astype(np.complex64), n, 0.5, win)
    # the smoke test's 1e-5 of the largest bin, plus what the bound of the float test can move a bin: mag_scale sum|window|
    mag_scale = orc.win_adj(win) * 2 / n
    tol = 1e-5 * want.max() + mag_scale * np.abs(win).sum() * dm.bound(taps, np.abs(x).max())
    assert np.max(np.abs(got - want)) <= tol, (np.max(np.abs(got - want)), tol)
    assert int(np.argmax(got)) == n // 2 + bin_in_span
    assert got[n // 2 + bin_in_span] > 0.9                                  # a pass-band tone of 0.5 still reads about 1.0
    eng.close()
    dc.close()


# ------------------------------------------------------------------------------------------ 7. command line
def test_cli_zoom_equals_the_classes(ksa, X, torch_cuda, tmp_path, capsys):
    K = importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")
    sources = importlib.import_module("prgs-sdr-kspecanal_amd.sources")
    n, frames, D, off = 1024, 8, 16, 300e3
    base = K.handle_args({}, ["zeroSpan", "fftSize", str(n), "zoom", "%d:%g" % (D, off), "iqFormat", "s16", "frameBatch", "4"])
    z, fs, full = base["zoom.spec"], base["samplingRate"], base["fullSize"]
    block_len = z["block_len"]
    assert block_len == D * (full - 1) + 8 * D
    settle = 16 * 1024                                 # the samples sdr_setup discards
    per_read = 1 << int(np.ceil(np.log2(block_len)))   # a block is one read, rounded up to a power of two and cut back (K:343)
    rng = np.random.default_rng(77)
    t = np.arange(settle + frames * per_read)
    x = 0.4 * np.exp(2j * np.pi * ((off + 20e3) / fs) * t) + 0.3 * np.exp(2j * np.pi * -0.31 * t) \
        + 0.02 * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
    raw = np.empty(2 * t.size, dtype=np.int16)
    raw[0::2] = np.round(x.real * 32767)
    raw[1::2] = np.round(x.imag * 32767)
    path = tmp_path / "cap_s16.bin"
    raw.tofile(path)
    common = ["zeroSpan", "fftSize", str(n), "zoom", "%d:%g" % (D, off), "iqFormat", "s16", "frameBatch", "4", "prgLoopCnt", str(frames),
              "source", "file:%s" % path, "bPltLevels", "false", "bPltHeatMap", "false"]

    # the same calls through the classes
    src = sources.FileSdr(str(path), iq_format="s16")
    src.read_samples(settle)
    blocks = np.array([K.sdr_read(src, block_len, raw="s16") for _ in range(frames)])
    src.close()
    assert blocks.shape == (frames, 2 * block_len) and blocks.dtype == np.int16
    assert np.array_equal(blocks[1], raw[2 * (settle + per_read):2 * (settle + per_read + block_len)])
    dc = X.DownConverter(ksa.FMT_S16, D, X.ddc_lowpass(D, 8), freq=off, sampling_rate=fs, max_in=4 * block_len)
    eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=base["curScanNonOverlap"], window=base["theWin"],
                             cumu_mode=base["curScanCumuMode"], gain=base["gain"], min_amp=base["minAmp4Clip"],
                             xres=base["xRes"], max_frames=4)
    for b in range(0, frames, 4):
        dc.blocks_dev(to_dev(torch_cuda, np.ascontiguousarray(blocks[b:b + 4]).reshape(-1)), 4, block_len)
        eng.frames_dev(dc.out_ptr, ksa.FMT_C64, 4)
        eng.synchronize()
    want = eng.state()
    eng.close()
    dc.close()

    def run(extra):
        K.sdr_curscan = K._gpu_curscan
        capsys.readouterr()
        d = K.main(common + extra)
        return d, capsys.readouterr().out

    d, out = run([])
    for k in ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg", "fftHM"):
        assert np.array_equal(d[k], want[k]), k                              # bit for bit
    freqs = d["freqs"]
    centre = base["centerFreq"] + off
    assert len(freqs) == n and freqs[0] == centre - fs / D / 2 and abs(freqs[-1] - (centre + fs / D / 2 - fs / D / n)) < 1e-3
    assert d["startFreq"] == centre - fs / D / 2 and d["endFreq"] == centre + fs / D / 2
    assert abs(freqs[int(np.argmax(d["Fft.Cur"]))] - (centre + 20e3)) <= fs / D / n     # the tone, 20 kHz above the zoom's centre
    assert "INFO: zoom [16]" in out
    both, _ = run(["density", "64:-120:0", "mask", "flat:1000"])
    for k in ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg", "fftHM"):
        assert np.array_equal(both[k], want[k]), k
    assert both["densityRows"] == frames and both["maskRows"] == frames and both["maskEventsTotal"] == 0
    one, _ = run(["frameBatch", "1"])                                        # a batch of one
    assert one["fftHMIndex"] == frames and np.array_equal(one["freqs"], freqs)
    assert np.allclose(one["Fft.Cur"], want["Fft.Cur"], rtol=0, atol=1e-3)   # dB; the last frame's own spectrum
