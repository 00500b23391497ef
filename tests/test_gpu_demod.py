"""The demodulator on the GPU against tests/demod_model.py (whose float32 emulation is checked against the bound on the CPU, in
tests/test_demod_host.py).  Shapes (D, T) take every tile the plan picks (1024 outputs, four per thread; 256; 64), the
largest span and a filter with fewer taps than the decimation ((8, 3): whole input samples lie between two outputs' spans); input lengths sit on every edge of the loader and the tile: 1, 2, D-1, D, D+1, T-1, T, one tile of outputs
+-1, three tiles + 5, and once from a pointer offset by one sample (8 mod 16).  Exact inputs are compared with
np.array_equal, floats against the bound written down in demod_model.bound."""
import importlib
import subprocess
import sys
import wave

import numpy as np
import pytest

import demod_model as mm
from conftest import ROOT, load_pkg

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 33), (2, 16), (3, 11), (8, 3), (5, 80), (64, 1024), (256, 4096)]
TILES = {(1, 1): 1024, (1, 33): 1024, (2, 16): 1024, (3, 11): 1024, (8, 3): 1024, (5, 80): 1024, (64, 1024): 256, (256, 4096): 64}
MODES = (mm.MODE_AM, mm.MODE_FM, mm.MODE_PM)
NAMES = {mm.MODE_AM: "am", mm.MODE_FM: "fm", mm.MODE_PM: "pm"}
WORST = {}                                   # (D, T) -> worst error / bound of the float test, printed at the end


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def X():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.demod")


def lengths_for(shape):
    """Input lengths on every edge of the loader and the tile."""
    D, T = shape
    t = TILES[shape]
    tile = D * (t - 1) + 1                                  # the shortest input that yields one tile of outputs
    return sorted({n for n in (1, 2, D - 1, D, D + 1, T - 1, T, tile - D, tile, tile + D, D * (3 * t + 4) + 1) if n >= 1})


def lowpass(X, D, T):
    """demod_taps where T is a whole number of phases, else the same formula at that T."""
    if T % D == 0:
        return X.demod_taps(D, T // D)
    t = np.arange(T, dtype=np.float64) - (T - 1) / 2
    h = np.sinc(0.8 * t / D) * np.hamming(T)
    return (h / h.sum()).astype(np.float32)


def to_dev(torch, x, offset=0):
    """(tensor that owns the memory, device address of the samples): complex64 on the device, `offset` samples into an
    allocation, so that offset 1 puts the first sample at 8 mod 16."""
    buf = torch.zeros(2 * (len(x) + offset + 1), dtype=torch.float32, device="cuda")
    buf[2 * offset:2 * (offset + len(x))] = torch.from_numpy(np.ascontiguousarray(x).view(np.float32))
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + 8 * offset


def run_stream(torch, dm, x, offset=0):
    """x through process_dev into a caller's buffer; float32 or int16 on the host."""
    want = dm.out_count(len(x))
    out = torch.zeros(max(want, 1), dtype=torch.int16 if dm.dtype == np.int16 else torch.float32, device="cuda")
    keep, ptr = to_dev(torch, x, offset)
    got = dm.process_dev(ptr if len(x) else 0, len(x), out=out, out_capacity=want)
    assert got == want
    dm.synchronize()
    del keep
    return out[:got].cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16)


def exact_input(rng, n, mode):
    """(complex64 [n], exact detector numerators, denominator, k or None)."""
    if mode == mm.MODE_AM:
        x, mag = mm.exact_am_samples(rng, n)
        return (x,) + mm.exact_detect(mode, mag=mag) + (None,)
    x, k = mm.exact_turn_samples(rng, n)
    return (x,) + mm.exact_detect(mode, k=k) + (k,)


# ------------------------------------------------------------------------------------------ 1. exact
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_impulse_places_every_tap_exactly(X, torch_cuda, shape):
    D, T = shape
    rng = np.random.default_rng(D * 100003 + T)
    taps = rng.uniform(-1, 1, T).astype(np.float32)
    t = TILES[shape]
    count = t + 2
    n_in = D * (count - 1) + 1
    spots = {1, 2, D - 1, D, D + 1, T - 1, T, t * D - (T - 1) - 1, t * D - (T - 1), t * D - (T - 1) + 1, t * D - 1, t * D, t * D + 1, n_in - 1}
    for mode in MODES:
        dm = X.Demodulator(mode, D, taps, max_in=1 << 18)
        assert dm.kernel_info()["tile_out"] == t
        for p in sorted(s for s in spots if 1 <= s < n_in):
            x = np.zeros(n_in, dtype=np.complex64)            # d[p] = c, every other d[n] = 0
            if mode == mm.MODE_AM:
                x[p], c = -1j, np.float32(1)
            elif mode == mm.MODE_PM:
                x[p], c = -2j, np.float32(-0.25)
            else:
                x[p - 1], x[p], c = 3, -2j, np.float32(-0.25)
            dm.reset()
            y = dm.process(x)
            k = np.arange(count) * D - p
            want = np.where((k >= 0) & (k < T), taps[np.clip(k, 0, T - 1)] * c, np.float32(0)).astype(np.float32)
            assert y.shape == (count,) and np.array_equal(y, want), (shape, mode, p)
        dm.close()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_exact_inputs_in_every_mode_format_and_form(X, torch_cuda, shape):
    D, T = shape
    rng = np.random.default_rng(D * 7919 + T)
    taps = rng.integers(-8, 9, T).astype(np.float64)
    taps[0], taps[-1] = 8, -7                              # the outermost taps are there
    if T >= 4:
        taps[1], taps[2] = 0.5, -0.25                      # powers of two among the small integers
    lengths = lengths_for(shape)
    t = TILES[shape]
    ends = set()
    for mode in MODES:
        x, dn, dden, k = exact_input(rng, lengths[-1] + 1, mode)
        # int16 per unit, from the model: the median of the non-zero |y| lands in the upper half of [32768, 65536), so that
        # at least half of them saturate and whatever lies below half the median does not
        conv = mm.exact_conv(dn, dden, taps)               # once: every length and block picks from it
        y = np.abs(mm.exact_stream(dn[:lengths[-1]], dden, taps, D, conv=conv).astype(np.float64))
        pcm_scale = 2.0 ** np.ceil(np.log2(32768 / np.median(y[y > 0])))
        for fmt, name in ((mm.OUT_F32, "f32"), (mm.OUT_S16, "s16")):
            dm = X.Demodulator(NAMES[mode], D, taps, out_fmt=name, pcm_scale=pcm_scale, max_in=1 << 18)
            for n, offset in [(n, 0) for n in lengths] + [(lengths[-1], 1)]:       # the longest once more, from a pointer at 8 mod 16
                want = mm.exact_stream(dn[:n], dden, taps, D, fmt, pcm_scale, conv=conv)
                dm.reset()
                got = run_stream(torch_cuda, dm, x[:n], offset)
                assert got.dtype == want.dtype and np.array_equal(got, want), (shape, mode, name, n, offset, "stream")
                if fmt == mm.OUT_S16 and n == lengths[-1]:
                    ends.update(int(v) for v in (got.min(), got.max()))
                    assert np.any(np.abs(got.astype(np.int32)) < 32767) and np.any(np.abs(got.astype(np.int32)) >= 32767), (shape, mode)
            # the block form: three overlapping blocks of M outputs each, from either alignment
            for M in (1, t + 1):
                L = mm.lead(mode) + D * (M - 1) + T
                stride = max(1, L // 2) | 1                 # odd: the blocks start at 0 and at 8 mod 16
                starts = [0, stride, 2 * stride]
                wantb = mm.exact_blocks(dn, dden, taps, D, mode, starts, L, fmt, pcm_scale, conv=conv)
                keep, ptr = to_dev(torch_cuda, x[:2 * stride + L])
                assert dm.blocks_dev(ptr, 3, L, block_stride=stride) == M == dm.block_out_count(L)
                got = dm.read_out(3 * M).reshape(3, M)
                assert np.array_equal(got, wantb), (shape, mode, name, M, "blocks")
                assert np.array_equal(torch_cuda.as_tensor(dm.out, device="cuda")[:3 * M].cpu().numpy().reshape(3, M), wantb)
                del keep
            dm.close()
    assert {-32768, 32767} <= ends, (shape, ends)          # int16 saturates at both ends


# ------------------------------------------------------------------------------------------ 2. cuts
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_the_cut_of_the_stream_does_not_show(X, torch_cuda, shape):
    D, T = shape
    rng = np.random.default_rng(D * 271 + T)
    taps = lowpass(X, D, T)
    t = TILES[shape]
    for mode in MODES:
        dm = X.Demodulator(mode, D, taps, max_in=1 << 18)
        cuts = [1, 0, D - 1, D, 1, max(T - 2, 0), T - 1, T, 0, D * (2 * t + 5) + 3] + [int(c) for c in rng.integers(0, 3 * D + 3, 6)]
        cuts = [cuts[i] for i in rng.permutation(len(cuts))]
        n = sum(cuts)
        x = mm.float_input(rng, n, mode)
        whole = run_stream(torch_cuda, dm, x)
        assert dm.state() == {"samples_in": n, "samples_out": len(whole)} and len(whole) == -(-n // D)
        dm.reset()
        assert dm.state() == {"samples_in": 0, "samples_out": 0}
        parts, at = [], 0
        for i, c in enumerate(cuts):
            assert dm.out_count(c) == mm.out_count(at, c, D)
            parts.append(run_stream(torch_cuda, dm, x[at:at + c], offset=i & 1))
            assert len(parts[-1]) == mm.out_count(at, c, D)
            at += c
        assert np.array_equal(bits(np.concatenate(parts)), bits(whole)), (shape, mode)            # bit for bit
        # the host entry point agrees, and reset restores the start
        dm.reset()
        assert np.array_equal(bits(dm.process(x)), bits(whole))
        dm.reset()
        assert np.array_equal(bits(run_stream(torch_cuda, dm, x)), bits(whole))
        # set_taps keeps the history: the outputs after it are those of a stream that had the new taps all along
        half = n // 2 + 1
        taps2 = (taps[::-1] * np.float32(0.5) + np.float32(0.01)).astype(np.float32)
        dm.reset()
        a = dm.process(x[:half])
        dm.set_taps(taps2)
        b = dm.process(x[half:])
        other = X.Demodulator(mode, D, taps2, max_in=1 << 18)
        ref = other.process(x)
        other.close()
        assert np.array_equal(bits(a), bits(whole[:len(a)])) and np.array_equal(bits(b), bits(ref[len(a):])), (shape, mode)
        dm.close()


# ------------------------------------------------------------------------------------------ 3. blocks
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_block_form_is_the_stream_form_past_its_transient(X, torch_cuda, shape):
    torch = torch_cuda
    D, T = shape
    rng = np.random.default_rng(D * 977 + T)
    taps = lowpass(X, D, T)
    t = TILES[shape]
    M = t + 1
    for mode in MODES:
        ld = mm.lead(mode)
        L = ld + D * (M - 1) + T + (D - 1)                 # the last D - 1 samples yield no further output
        stride = L - min(L - 1, 2 * D + 1)                 # the blocks overlap
        nblocks = 3
        x = mm.float_input(rng, stride * (nblocks - 1) + L, mode)
        dm = X.Demodulator(mode, D, taps, max_in=1 << 18)
        dm.process(mm.float_input(rng, 3 * D + 1, mode))   # a stream is under way: the block form must not touch it
        state = dm.state()
        keep, ptr = to_dev(torch, x)
        assert dm.blocks_dev(ptr, nblocks, L, block_stride=stride) == M
        own = dm.read_out(nblocks * M).reshape(nblocks, M)
        out = torch.full((nblocks, M + 3), 7.0, dtype=torch.float32, device="cuda")
        dm.blocks_dev(ptr, nblocks, L, block_stride=stride, out=out, out_stride=M + 3)
        dm.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(bits(got[:, :M]), bits(own)) and np.all(got[:, M:] == 7.0)          # the gaps are untouched
        assert dm.state() == state
        # a stream fed zeros and then the block: block output m is stream output (pad + lead + m D + T-1) / D
        pad = -(ld + T - 1) % D
        st = X.Demodulator(mode, D, taps, max_in=1 << 18)
        for b in range(nblocks):
            st.reset()
            y = st.process(np.concatenate([np.zeros(pad, dtype=np.complex64), x[b * stride:b * stride + L]]))
            j0 = (pad + ld + T - 1) // D
            assert np.array_equal(bits(y[j0:j0 + M]), bits(own[b])), (shape, mode, b)
        st.close()
        dm.close()
        del keep


# ------------------------------------------------------------------------------------------ 4. floats, bounded
def check_bound(got, want, taps, mode, max_abs, shape, what):
    limit = mm.bound(taps, mode, max_abs)
    worst = float(np.max(np.abs(got.astype(np.float64) - want))) / limit if len(got) else 0.0
    WORST[shape] = max(WORST.get(shape, 0.0), worst)
    print("demod float test %s mode %d %s: worst error / bound = %.4f" % (shape, mode, what, worst))
    assert got.shape == want.shape and worst <= 1.0, (shape, mode, what, worst)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_floats_stay_inside_the_bound(X, torch_cuda, shape):
    D, T = shape
    rng = np.random.default_rng(D * 31337 + T)
    taps = lowpass(X, D, T)
    t = TILES[shape]
    for mode in MODES:
        dm = X.Demodulator(mode, D, taps, max_in=1 << 18)
        for count, offset in ((t + 1, 1), (3 * t + 5, 0)):
            n = D * (count - 1) + 1
            x = mm.float_input(rng, n, mode)
            want = mm.fir_at(mm.detect(x, mode), taps, D, 0, count)
            dm.reset()
            check_bound(run_stream(torch_cuda, dm, x, offset), want, taps, mode, np.abs(x).max(), shape, "stream %d" % count)
        M = t + 1
        L = mm.lead(mode) + D * (M - 1) + T
        x = mm.float_input(rng, 2 * L, mode).reshape(2, L)
        want = np.array([mm.fir_at(mm.detect(row, mode), taps, D, mm.lead(mode) + T - 1, M) for row in x])
        keep, ptr = to_dev(torch_cuda, x.reshape(-1))
        assert dm.blocks_dev(ptr, 2, L) == M
        check_bound(dm.read_out(2 * M).reshape(2, M), want, taps, mode, np.abs(x).max(), shape, "blocks")
        dm.close()
        del keep


def test_detector_alone_near_half_a_turn(X, torch_cuda):
    """D = 1, T = 1, h = [1]: the detector's own error, with steps (FM) and phases (PM) within 1e-6 of +-0.5 turn, by circular
    distance against B alone.  AM is held, sample by sample, to 4 units of its own |x|: the two roundings of the square move it
    by at most 2 units relative, the root halves that and adds half a unit of its own."""
    rng = np.random.default_rng(1234)
    n = 8192
    ang = rng.uniform(-0.5, 0.5, n)
    ang[:2048] = rng.choice([-0.5, 0.5], 2048) + rng.uniform(-1e-6, 1e-6, 2048)
    amp = np.exp(rng.uniform(np.log(1e-3), np.log(3e4), n))
    for mode in (mm.MODE_FM, mm.MODE_PM):
        x = (amp * np.exp(2j * np.pi * (np.cumsum(ang) if mode == mm.MODE_FM else ang))).astype(np.complex64)
        dm = X.Demodulator(mode, 1, np.ones(1, dtype=np.float32), max_in=n)
        got = run_stream(torch_cuda, dm, x).astype(np.float64)
        dm.close()
        assert np.all(np.abs(got) <= 0.5)
        e = got - mm.detect(x, mode)
        e = np.abs(e - np.round(e))
        worst = e.max() / mm.detector_units(mode, 1.0)
        WORST[("detector", mode)] = worst
        print("demod detector test mode %d: worst circular error / B = %.4f" % (mode, worst))
        assert worst <= 1.0, (mode, worst)
    x = (amp * np.exp(2j * np.pi * ang)).astype(np.complex64)
    dm = X.Demodulator(mm.MODE_AM, 1, np.ones(1, dtype=np.float32), max_in=n)
    got = run_stream(torch_cuda, dm, x).astype(np.float64)
    dm.close()
    worst = np.max(np.abs(got - mm.detect(x, mm.MODE_AM)) / (4 * mm.UNIT * np.abs(x)))     # per sample: relative to its own |x|
    WORST[("detector", mm.MODE_AM)] = worst
    print("demod detector test mode 0: worst error / (4 units of |x|) = %.4f" % worst)
    assert worst <= 1.0, worst


def test_nan_becomes_zero_in_int16_output(X, torch_cuda):
    """Finite input reaches a NaN sum: AM samples whose square overflows float32 give d = inf, and taps [1, -1] then give
    inf - inf.  int16 stores 0 for it, not an end of the scale; the first stream output, inf alone, saturates."""
    x = np.full(2100, 3e19, dtype=np.complex64)
    taps = np.array([1, -1], dtype=np.float32)
    f32 = X.Demodulator("am", 1, taps, max_in=4096)
    y = run_stream(torch_cuda, f32, x)
    assert y[0] == np.inf and np.all(np.isnan(y[1:]))                        # the premise
    f32.close()
    dm = X.Demodulator("am", 1, taps, out_fmt="s16", pcm_scale=1.0, max_in=4096)
    got = run_stream(torch_cuda, dm, x)
    assert got.shape == (2100,) and got[0] == 32767 and not np.any(got[1:]), got[:4]
    keep, ptr = to_dev(torch_cuda, x)
    assert dm.blocks_dev(ptr, 2, 1050) == 1049
    assert not np.any(dm.read_out(2 * 1049))
    dm.close()
    del keep


def test_a_later_smaller_object_does_not_lower_the_lds_limit(X, torch_cuda):
    """The dynamic-LDS limit belongs to the kernel function, and (64, 1024) and (10, 1) both run tile_kernel<AM, 1, float>, with
    68 KiB and 10 KiB: the larger object, made first, still launches after the smaller one was made."""
    rng = np.random.default_rng(4242)
    big = X.Demodulator("am", 64, lowpass(X, 64, 1024), max_in=1 << 18)
    small = X.Demodulator("am", 10, np.ones(1, dtype=np.float32), max_in=1 << 18)
    assert big.kernel_info()["tile_out"] == small.kernel_info()["tile_out"] == 256
    assert big.kernel_info()["lds_bytes"] > 65536 > small.kernel_info()["lds_bytes"]
    x = mm.float_input(rng, 64 * 300 + 1, mm.MODE_AM)
    want = mm.fir_at(mm.detect(x, mm.MODE_AM), big.taps, 64, 0, 301)
    check_bound(run_stream(torch_cuda, big, x), want, big.taps, mm.MODE_AM, np.abs(x).max(), (64, 1024), "after a smaller object")
    small.close()
    big.close()


def test_report_the_worst_ratio():
    print("demod float test: worst error / bound per shape:", {k: round(v, 4) for k, v in WORST.items()})
    assert all(v <= 1.0 for v in WORST.values())


# ------------------------------------------------------------------------------------------ 5. behind the down-converter
def test_chain_from_the_down_converter_without_a_synchronise(X, torch_cuda):
    torch = torch_cuda
    ddc = importlib.import_module("prgs-sdr-kspecanal_amd.ddc")
    zoomD, full, nblocks, D = 8, 2048, 3, 5
    ztaps = ddc.ddc_lowpass(zoomD, 8)
    block_len = zoomD * (full - 1) + len(ztaps)
    f0, dev, fm = 0.11, 0.02, 0.0007                       # carrier, peak deviation, modulating tone: cycles per input sample
    tt = np.arange(nblocks * block_len)
    x = (0.5 * np.exp(2j * np.pi * (f0 * tt - dev / fm * np.cos(2 * np.pi * fm * tt) / (2 * np.pi)))).astype(np.complex64)
    stream = torch.cuda.Stream()
    dc = ddc.DownConverter(ddc.FMT_C64, zoomD, ztaps, phase_inc=ddc.phase_inc_for(f0, 1.0), max_in=nblocks * block_len,
                           stream=stream.cuda_stream)
    taps = X.demod_taps(D, 8)
    dm = X.Demodulator("fm", D, taps, max_in=nblocks * full, stream=stream.cuda_stream)
    keep, ptr = to_dev(torch, x)
    torch.cuda.synchronize()
    assert dc.blocks_dev(ptr, nblocks, block_len) == full
    M = dm.blocks_dev(dc.out_ptr, nblocks, full)           # no synchronisation in between: one stream orders them
    got = dm.read_out(nblocks * M).reshape(nblocks, M)
    z = torch.as_tensor(dc.out, device="cuda")[:nblocks * full].cpu().numpy().reshape(nblocks, full)
    want = mm.blocks(z, taps, D, mm.MODE_FM)
    assert want.shape == (nblocks, M)
    check_bound(got, want, taps, mm.MODE_FM, np.abs(z).max(), ("chain", D, len(taps)), "blocks")
    assert abs(np.abs(want).max() - zoomD * dev) < 0.02 * zoomD * dev       # the deviation, in cycles per zoomed sample
    dm.close()
    dc.close()
    del keep


# ------------------------------------------------------------------------------------------ 6. refusals, kernel_info
def test_refusals_per_call_leave_the_object_as_it_was(X, torch_cuda):
    torch = torch_cuda
    D, T = 3, 11
    taps = lowpass(X, D, T)
    rng = np.random.default_rng(99)
    dm = X.Demodulator("fm", D, taps, max_in=4096)
    x = mm.float_input(rng, 100, mm.MODE_FM)
    first = dm.process(x)
    keep, ptr = to_dev(torch, x)
    dm.blocks_dev(ptr, 2, 50)
    before, state = dm.read_out(dm.out_capacity), dm.state()
    small = torch.zeros(4, dtype=torch.float32, device="cuda")
    texts = []
    for call, text in ((lambda: dm.process_dev(0, 5), "null input pointer"),
                       (lambda: dm.process_dev(ptr + 4, 5), "not aligned"),
                       (lambda: dm.process_dev(ptr, -1), "n_in -1 must be >= 0"),
                       (lambda: dm.process_dev(ptr, 4097), "exceeds max_in"),
                       (lambda: dm.process_dev(ptr, 100, out=small, out_capacity=4), "output capacity 4 is too small"),
                       (lambda: dm.blocks_dev(0, 2, 50), "null input pointer"),
                       (lambda: dm.blocks_dev(ptr + 4, 2, 50), "not aligned"),
                       (lambda: dm.blocks_dev(ptr, -1, 50), "nblocks -1 must be >= 0"),
                       (lambda: dm.blocks_dev(ptr, 2, 50, block_stride=-1), "block_stride -1 must be >= 0"),
                       (lambda: dm.blocks_dev(ptr, 2, T), "shorter than the"),
                       (lambda: dm.blocks_dev(ptr, 100, 50), "exceed max_in"),
                       (lambda: dm.blocks_dev(ptr, 2, 50, out=small, out_stride=3), "out_stride 3 is shorter"),
                       (lambda: dm.read_out(5, first=-1), "first -1"), (lambda: dm.read_out(-5), "count -5"),
                       (lambda: dm.read_out(2, first=dm.out_capacity - 1), "outside the output buffer")):
        with pytest.raises(X.KsaError, match=text):
            call()
        texts.append(text)
    assert dm.block_out_count(T + 1) == 1 and dm.blocks_dev(ptr, 0, T + 1) == 1          # the shortest block; no blocks: a no-op
    assert dm.process_dev(0, 0) == 0                       # n_in = 0 is a successful no-op, whatever the pointer
    assert dm.state() == state and np.array_equal(bits(dm.read_out(dm.out_capacity)), bits(before))
    tail = mm.float_input(rng, 20, mm.MODE_FM)
    fresh = X.Demodulator("fm", D, taps, max_in=4096)
    assert np.array_equal(bits(fresh.process(x)), bits(first))
    assert np.array_equal(bits(dm.process(tail)), bits(fresh.process(tail)))             # the history too
    fresh.close()
    dm.close()
    del keep


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_kernel_info_is_consistent(X, torch_cuda, shape):
    D, T = shape
    dm = X.Demodulator("am", D, np.ones(T, dtype=np.float32), max_in=1 << 18)
    info = dm.kernel_info()
    t = info["tile_out"]
    span = (t - 1) * D + T
    assert t == TILES[shape] and info["threads"] == 256 and info["grid"] >= 1 and 0 < info["vgprs"] <= 128
    assert span * 4 <= info["lds_bytes"] <= (span + 2 * D) * 4 <= 160 * 1024
    n = D * (2 * t) + 1
    dm.process_dev(to_dev(torch_cuda, np.ones(n, dtype=np.complex64))[1], n)
    dm.synchronize()
    assert dm.kernel_info()["grid"] == 3                   # 2 t + 1 outputs: three tiles
    dm.close()


# ------------------------------------------------------------------------------------------ 7. command line
def test_cli_demodulates_an_fm_tone_into_a_wav_file(tmp_path):
    K = importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")
    fs, off, tone, dev, amp = 2.4e6, 300e3, 1e3, 5e3, 0.5
    n_fft, frames = 1024, 4
    base = K.handle_args({}, ["zeroSpan", "fftSize", str(n_fft), "iqFormat", "s16", "zoom", "10:300e3", "demod", "fm:5"])
    block_len, per_block = base["zoom.spec"]["block_len"], base["demod.spec"]["out_per_block"]
    per_read = 1 << int(np.ceil(np.log2(block_len)))        # a block is one read, rounded up to a power of two and cut back
    t = np.arange(16 * 1024 + frames * per_read) / fs
    x = amp * np.exp(1j * (2 * np.pi * off * t + dev / tone * np.sin(2 * np.pi * tone * t)))
    raw = np.empty(2 * t.size, dtype=np.int16)
    raw[0::2] = np.round(x.real * 32767)
    raw[1::2] = np.round(x.imag * 32767)
    path, wav = tmp_path / "fm_s16.bin", tmp_path / "out.wav"
    raw.tofile(path)
    r = subprocess.run([sys.executable, "-m", "prgs-sdr-kspecanal_amd.kspecanal", "zeroSpan", "fftSize", str(n_fft), "iqFormat", "s16",
                        "zoom", "10:300e3", "demod", "fm:5", "demodSave", str(wav), "source", "file:%s" % path, "prgLoopCnt", str(frames),
                        "bPltLevels", "false", "bPltHeatMap", "false"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "INFO: demod [fm]" in r.stdout and "INFO:zero_span: demod [fm]" in r.stdout
    with wave.open(str(wav), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 48000)
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.float64)
    assert pcm.shape == (frames * per_block,)
    want = dev / (fs / 10) * K.DEMOD_PCM_SCALE
    tt = np.arange(per_block) / 48000.0
    basis = np.stack([np.cos(2 * np.pi * tone * tt), np.sin(2 * np.pi * tone * tt)], axis=1)
    for b, y in enumerate(pcm.reshape(frames, per_block)):
        coef = np.linalg.lstsq(basis, y, rcond=None)[0]
        got = float(np.hypot(coef[0], coef[1]))
        rms = float(np.sqrt(np.mean((y - basis @ coef) ** 2)))
        print("demod cli block %d: amplitude %.2f (want %.2f), residual rms %.3f" % (b, got, want, rms))
        assert abs(got - want) <= 0.01 * want and rms < 0.02 * want, (b, got, want, rms)
