"""The polyphase channelizer on the GPU against tests/chan_model.py (whose polyphase evaluation is checked against the
definition, and whose float32 emulation against the bound, on the CPU in tests/test_chan_host.py).  Shapes (M, O, P) cover both
parities of log2 M, D = 1, transforms of one wave and of the whole workgroup, and the largest span; input lengths sit on every
edge of the loader and either side of a workgroup's tile of columns (kernel_info's tile_cols).  Impulses and integers are
compared exactly, floats against chan_model.bound."""
import importlib

import numpy as np
import pytest

import chan_model as cm
import ddc_model as dm
import demod_model as mm
from conftest import load_pkg

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 1), (2, 2, 3), (4, 4, 2), (8, 2, 3), (16, 1, 4), (64, 4, 2), (32, 1, 32), (256, 2, 8), (512, 2, 16), (1024, 1, 8),
          (1024, 4, 8)]
FMTS = (cm.FMT_C64, cm.FMT_U8, cm.FMT_S8, cm.FMT_S16)
MAX_IN = 1 << 18
WORST = {}                                   # (M, O, P) -> worst error / bound of the float test, printed at the end


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def X():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.chan")


def proto(X, M, P, cutoff=1.0):
    return X.chan_prototype(M, P, cutoff)


def lengths_for(ch):
    """Input lengths on the loader's and the tile's edges: 1, 2, D-1, D, D+1, T-1, T, a tile of columns -+ one, three tiles + 5."""
    D, T, W = ch.decim, ch.ntaps, ch.kernel_info()["tile_cols"]
    cols = (W - 1, W, W + 1, 3 * W + 5)
    return sorted({n for n in (1, 2, D - 1, D, D + 1, T - 1, T) + tuple(D * (c - 1) + 1 for c in cols) if 1 <= n <= MAX_IN})


def random_raw(rng, fmt, n):
    if fmt == cm.FMT_C64:
        return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)
    info = {cm.FMT_U8: (0, 256, np.uint8), cm.FMT_S8: (-128, 128, np.int8), cm.FMT_S16: (-32768, 32768, np.int16)}[fmt]
    return rng.integers(info[0], info[1], 2 * n).astype(info[2])


def int_raw(rng, fmt, n, amp):
    """Raw samples whose integer values stay within +-amp (uint8: around 128; complex64: k / 2^15)."""
    b = rng.integers(-amp, amp + 1, 2 * n)
    if fmt == cm.FMT_C64:
        return ((b[0::2] + 1j * b[1::2]) / 32768.0).astype(np.complex64)
    if fmt == cm.FMT_U8:
        return (b + 128).astype(np.uint8)
    return b.astype(np.int8 if fmt == cm.FMT_S8 else np.int16)


def to_dev(torch, raw, lead=0):
    """(owner, device tensor of raw) with the samples `lead` samples into their allocation."""
    per = 1 if raw.dtype == np.complex64 else 2
    flat = raw.view(np.float32) if raw.dtype == np.complex64 else raw
    unit = 2 if raw.dtype == np.complex64 else per
    buf = torch.zeros(flat.size + lead * unit, dtype=torch.from_numpy(flat[:1]).dtype, device="cuda")
    buf[lead * unit:] = torch.from_numpy(flat).cuda()
    return buf, buf[lead * unit:]


def run_stream(torch, ch, raw, lo, n, lead=0, pad=3):
    """Samples [lo, lo + n) of raw through process_dev into a caller's buffer with `pad` spare values per channel, which must
    stay untouched; complex64 [M][columns] on the host."""
    per = 1 if raw.dtype == np.complex64 else 2
    want = ch.out_count(n)
    stride = want + pad
    out = torch.full((ch.nchan, max(stride, 1)), complex(7.0, -7.0), dtype=torch.complex64, device="cuda")
    keep, x = to_dev(torch, raw[per * lo:per * (lo + n)], lead)
    got = ch.process_dev(x, n, out=out, chan_stride=stride)
    assert got == want
    ch.synchronize()
    host = out.cpu().numpy()
    assert np.all(host[:, want:] == np.complex64(complex(7.0, -7.0))), "the gap between channels was written"
    return host[:, :want]


def unpacked(raw, fmt):
    return cm.unpack(raw, fmt, 128.0, 128.0)


def make(X, fmt, M, O, taps, **kw):
    return X.Channelizer(fmt, M, O, taps, max_in=MAX_IN, u8_offset=128.0, u8_scale=128.0, **kw)


# ------------------------------------------------------------------------------------------ 1. impulse, exact
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_impulse_places_every_tap_exactly(X, torch_cuda, shape):
    M, O, P = shape
    rng = np.random.default_rng(M * 1009 + O * 31 + P)
    taps = rng.uniform(-1, 1, M * P).astype(np.float32)
    ch = make(X, cm.FMT_C64, M, O, taps)
    D, T, W = ch.decim, ch.ntaps, ch.kernel_info()["tile_cols"]
    for n_in in lengths_for(ch):
        spots = {0, 1, D - 1, D, M, T - 1, T, n_in - 1, W * D - (T - 1), W * D - 1, W * D, 2 * M, (n_in - 1) // M * M}
        for n0 in sorted(s for s in spots if 0 <= s < n_in):
            x = np.zeros(n_in, dtype=np.complex64)
            x[n0] = 1j
            ch.reset()
            y = ch.process(x)
            cols = -(-n_in // D)
            k = np.arange(cols) * D - n0
            want = np.where((k >= 0) & (k < T), taps[np.clip(k, 0, T - 1)], np.float32(0)).astype(np.complex64) * np.complex64(1j)
            assert y.shape == (M, cols) and np.array_equal(y[0], want), (shape, n_in, n0)
            if n0 % M == 0:
                assert np.array_equal(y, np.broadcast_to(want, (M, cols))), (shape, n_in, n0)
    ch.close()


# ------------------------------------------------------------------------------------------ 2. integers, exact
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_integers_are_exact_on_the_axis_channels_in_every_format(X, torch_cuda, shape):
    """Taps in -3 .. 3 (the outermost non-zero) and samples within +-amp / scale keep every partial sum an integer multiple of
    1 / scale below 2^24, so float32 is exact; channels 0, M/4, M/2 and 3M/4 only meet the twiddles (1,0) and (0,1)."""
    torch = torch_cuda
    M, O, P = shape
    T, D = M * P, M // O
    rng = np.random.default_rng(M * 7001 + O * 13 + P)
    taps = rng.integers(-3, 4, T)
    taps[0], taps[-1] = 2, -3
    first = cm.first_column(M, O, P)
    for fmt in FMTS:
        ch = make(X, fmt, M, O, taps.astype(np.float32))
        W = ch.kernel_info()["tile_cols"]
        amp = min(100, 2 ** 23 // (3 * T))                       # 3 T amp < 2^23
        n = D * (first + 3 * W + 4) + 1
        raw = int_raw(rng, fmt, n, amp)
        iq, scale = cm.to_int(raw, fmt)
        y = run_stream(torch, ch, raw, 0, n)
        cols = np.arange(y.shape[1])
        chans = sorted({0, M // 2} | ({M // 4, 3 * M // 4} if M >= 4 else set()))
        for c in chans:
            assert np.array_equal(y[c], cm.int_channel(iq, scale, taps, M, O, c, cols)), (shape, fmt, c)
        # the block form: two overlapping blocks into the object's own buffer, and the level meter on exact values.  A block's
        # mixer starts at the block's first sample, so blocks M samples (O columns) apart see the stream's phases.
        L = ch.block_len_for(W + 2)
        assert 2 * L <= MAX_IN and L + M <= n
        keep, x = to_dev(torch, raw)
        assert ch.blocks_dev(x, 2, L, block_stride=M) == W + 2
        for b in range(2):
            for c in chans:
                got = ch.read_out(b * M + c, 0, W + 2)
                assert np.array_equal(got, y[c, first + b * O:first + b * O + W + 2]), (shape, fmt, b, c)
        power = ch.channel_power(0, W + 2)
        for c in chans:
            v = np.concatenate([y[c, first + b * O:first + b * O + W + 2] for b in range(2)]).astype(np.complex128)
            assert power[c] == np.sum(v.real ** 2 + v.imag ** 2), (shape, fmt, c)       # integers over scale^2: exact in any order
        # blocks that start anywhere (odd starts are no multiple of M, and move the 16-byte loads over every alignment): each
        # equals the exact integer channelizer of its own samples, whose mixer starts at the block's first sample
        F, step = W + 1, 3
        L = ch.block_len_for(F)
        assert 3 * L <= MAX_IN and 1 + 2 * step + L <= n
        per = 1 if fmt == cm.FMT_C64 else 2
        keep, x = to_dev(torch, raw[per:], lead=2)
        out = torch.full((3, M, F + 1), complex(7.0, -7.0), dtype=torch.complex64, device="cuda")
        assert ch.blocks_dev(x, 3, L, block_stride=step, out=out, chan_stride=F + 1) == F
        ch.synchronize()
        got = out.cpu().numpy()
        assert np.all(got[:, :, F] == np.complex64(complex(7.0, -7.0)))
        for b in range(3):
            lo = 1 + b * step
            for c in chans:
                want = cm.int_channel(iq[lo:lo + L], scale, taps, M, O, c, np.arange(first, first + F))
                assert np.array_equal(got[b, c, :F], want), (shape, fmt, "block at", lo, c)
        ch.close()


# ------------------------------------------------------------------------------------------ 3. floats, inside the bound
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_floats_stay_inside_the_bound_in_every_format_and_both_forms(X, torch_cuda, shape):
    torch = torch_cuda
    M, O, P = shape
    D = M // O
    taps = proto(X, M, P)
    first = cm.first_column(M, O, P)
    worst = 0.0
    for fmt in FMTS:
        ch = make(X, fmt, M, O, taps)
        W = ch.kernel_info()["tile_cols"]
        n = D * (first + 3 * W + 4) + 1
        rng = np.random.default_rng(M * 31337 + O * 101 + P * 7 + fmt)
        raw = random_raw(rng, fmt, n)
        x = unpacked(raw, fmt)
        y = run_stream(torch, ch, raw, 0, n, lead=1)               # the input one sample into its allocation
        want = cm.polyphase(x, taps, M, O)
        b = cm.bound(taps, np.abs(x).max(), M, P)
        ratio = float(np.max(np.abs(y - want)) / b)
        worst = max(worst, ratio)
        assert y.shape == want.shape and ratio <= 1.0, (shape, fmt, ratio)
        # the block form on two blocks a prime stride apart
        F = W + 1
        L = ch.block_len_for(F)
        stride = 7 if D > 1 else 3
        assert L + stride <= n
        keep, xd = to_dev(torch, raw)
        out = torch.zeros((2, M, F + 2), dtype=torch.complex64, device="cuda")
        assert ch.blocks_dev(xd, 2, L, block_stride=stride, out=out, chan_stride=F + 2) == F
        ch.synchronize()
        got = out.cpu().numpy()
        assert np.all(got[:, :, F:] == 0)
        for blk in range(2):
            wb = cm.polyphase(x[blk * stride:blk * stride + L], taps, M, O, np.arange(first, first + F))
            ratio = float(np.max(np.abs(got[blk, :, :F] - wb)) / b)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (shape, fmt, blk, ratio)
        ch.close()
    WORST[shape] = worst
    print("chan float test %s: worst error / bound = %.4f" % (shape, worst))


# ------------------------------------------------------------------------------------------ 4. tone
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_a_tone_at_a_channel_centre_keeps_its_amplitude(X, torch_cuda, shape):
    """x[n] = exp(2 pi i c0 n / M) and non-negative taps: on channel c0 every term of the definition is h[k] >= 0, so
    |y| = sum h once the filter is full, and the bound is a relative 2^-24 (P + 4 log2 M + 16) -- tight enough to see a twiddle
    that is off by a few ulp, which random data (whose terms cancel) cannot."""
    M, O, P = shape
    D, T = M // O, M * P
    taps = np.abs(proto(X, M, P))
    ch = make(X, cm.FMT_C64, M, O, taps)
    W = ch.kernel_info()["tile_cols"]
    first = cm.first_column(M, O, P)
    n = D * (first + W + 2) + 1
    sumh = float(taps.astype(np.float64).sum())
    b = cm.bound(taps, 1.0, M, P)
    for c0 in sorted({c for c in (1, M // 2 - 1, M - 1) if 0 < c < M}):
        ph = (c0 * np.arange(n)) % M
        x64 = np.exp(2j * np.pi * ph / M)
        x = x64.astype(np.complex64)
        ch.reset()
        y = ch.process(x)
        want = cm.polyphase(x.astype(np.complex128), taps, M, O)
        full = y[c0, first:]
        rel = float(np.max(np.abs(np.abs(full.astype(np.complex128)) - sumh)) / b)
        print("chan tone test %s c0 %d: worst | |y| - sum h | / bound = %.4f" % (shape, c0, rel))
        assert rel <= 1.0, (shape, c0, rel)
        assert np.max(np.abs(y - want)) <= b, (shape, c0)
    ch.close()


# ------------------------------------------------------------------------------------------ 5. against the down-converter
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_channels_equal_a_down_converter_tuned_to_their_centre(X, torch_cuda, shape):
    torch = torch_cuda
    ddc = importlib.import_module("prgs-sdr-kspecanal_amd.ddc")
    M, O, P = shape
    D = M // O
    taps = proto(X, M, P)
    ch = make(X, cm.FMT_C64, M, O, taps)
    W = ch.kernel_info()["tile_cols"]
    n = D * (2 * W + 3) + 1
    rng = np.random.default_rng(M * 4241 + O * 17 + P)
    raw = random_raw(rng, cm.FMT_C64, n)
    keep, x = to_dev(torch, raw)
    cols = ch.process_dev(x, n)
    ch.synchronize()
    tol = cm.bound(taps, np.abs(raw).max(), M, P) + dm.bound(taps, np.abs(raw).max())
    for c in sorted({1, M // 2, M - 1}):
        dc = ddc.DownConverter(ddc.FMT_C64, D, taps, phase_inc=c * 2 ** 64 // M, max_in=MAX_IN)
        out = torch.zeros(cols, dtype=torch.complex64, device="cuda")
        assert dc.process_dev(x, n, out=out, out_capacity=cols) == cols
        dc.synchronize()
        assert np.max(np.abs(ch.read_out(c, 0, cols) - out.cpu().numpy())) <= tol, (shape, c)
        dc.close()
    ch.close()


# ------------------------------------------------------------------------------------------ 6. cuts
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_cuts_and_blocks_do_not_change_a_bit(X, torch_cuda, shape):
    torch = torch_cuda
    M, O, P = shape
    D, T = M // O, M * P
    taps = proto(X, M, P)
    first = cm.first_column(M, O, P)
    for fmt in (cm.FMT_C64, cm.FMT_S16):
        ch = make(X, fmt, M, O, taps)
        W = ch.kernel_info()["tile_cols"]
        n = D * (first + 3 * W + 4) + 1
        rng = np.random.default_rng(M * 911 + O * 3 + P + fmt)
        raw = random_raw(rng, fmt, n)
        whole = run_stream(torch, ch, raw, 0, n)
        assert ch.state() == {"samples_in": n, "samples_out": whole.shape[1]}
        for cuts in (sorted(set(rng.integers(1, n, 6).tolist())), sorted({c for c in (1, D - 1, D + 1, T - 1) if 0 < c < n})):
            ch.reset()
            parts, at = [], 0
            for edge in cuts + [n]:
                if edge > at:
                    parts.append(run_stream(torch, ch, raw, at, edge - at, lead=at % 3))
                    at = edge
            assert np.array_equal(np.concatenate(parts, axis=1), whole), (shape, fmt, cuts)
        # blocks: overlapping (stride < block_len), and stride 0.  A block's mixer starts at the block's first sample, so
        # blocks M samples (O columns) apart see the stream's phases.
        F = W + 1
        L = ch.block_len_for(F)
        keep, xd = to_dev(torch, raw)
        for stride, nb in ((M, 3), (0, 2)):
            assert nb * L <= MAX_IN and (nb - 1) * stride + L <= n
            assert ch.blocks_dev(xd, nb, L, block_stride=stride) == F and ch.layout() == (nb * M, F)
            ch.synchronize()
            got = torch.as_tensor(ch.out, device="cuda").cpu().numpy().reshape(nb, M, F)
            for b in range(nb):
                s = b * stride // D
                assert np.array_equal(got[b], whole[:, first + s:first + s + F]), (shape, fmt, stride, b)
        ch.close()


# ------------------------------------------------------------------------------------------ 7. strides and borders
def test_own_buffer_read_out_and_level_meter(X, torch_cuda):
    torch = torch_cuda
    M, O, P = 16, 2, 4
    taps = proto(X, M, P)
    ch = make(X, cm.FMT_C64, M, O, taps)
    n = 8 * 700 + 3
    raw = random_raw(np.random.default_rng(77), cm.FMT_C64, n)
    mine = run_stream(torch, ch, raw, 0, n, pad=11)                # a caller's stride beyond n_out: the gaps stay untouched
    ch.reset()
    keep, x = to_dev(torch, raw)
    cols = ch.process_dev(x, n)
    assert cols == mine.shape[1] and ch.layout() == (M, ch.out_stride) and ch.out_stride == -(-MAX_IN // 8) + 1
    ch.synchronize()
    own = torch.as_tensor(ch.out, device="cuda")[:, :cols].cpu().numpy()
    assert np.array_equal(own, mine)
    for c, lo, cnt in ((0, 0, cols), (5, 3, 100), (15, cols - 1, 1), (7, 10, 0)):
        assert np.array_equal(ch.read_out(c, lo, cnt), mine[c, lo:lo + cnt])
    for lo, cnt in ((0, cols), (3, 300), (cols - 1, 1), (5, 0)):
        v = mine[:, lo:lo + cnt].astype(np.complex128)
        want = np.sum(v.real ** 2 + v.imag ** 2, axis=1)
        got = ch.channel_power(lo, cnt)
        assert got.shape == (M,) and np.all(np.abs(got - want) <= 1e-12 * want), (lo, cnt)
    room = torch.zeros((M, 2 * cols), dtype=torch.complex64, device="cuda")     # large enough for any of these, were it not refused
    for bad, text in ((lambda: ch.read_out(M, 0, 1), "row 16"), (lambda: ch.read_out(-1, 0, 1), "row -1"),
                      (lambda: ch.read_out(0, ch.out_stride, 1), "outside"), (lambda: ch.channel_power(-1, 2), "outside"),
                      (lambda: ch.channel_power(0, ch.out_stride + 1), "outside"),
                      (lambda: ch.process_dev(x, n, out=room, chan_stride=ch.out_count(n) - 1), "chan_stride"),
                      (lambda: ch.process_dev(x, n, out=room, chan_stride=-1), "chan_stride"),
                      (lambda: ch.process_dev(x, MAX_IN + 1), "max_in"), (lambda: ch.process_dev(x.data_ptr() + 4, 8), "aligned"),
                      (lambda: ch.blocks_dev(x, 1, ch.block_len_for(1) - 1), "shorter"), (lambda: ch.blocks_dev(x, 2, MAX_IN), "max_in"),
                      (lambda: ch.blocks_dev(x, 1, 200, block_stride=-1), "block_stride"),
                      (lambda: ch.blocks_dev(x, 1, 200, out=room, chan_stride=16), "chan_stride")):
        with pytest.raises(X.KsaError, match=text):
            bad()
    assert ch.state() == {"samples_in": n, "samples_out": cols}    # refusals left the object as it was
    ch.close()


# ------------------------------------------------------------------------------------------ 8. state
def test_state_taps_reset_streams_and_shared_kernel(X, torch_cuda):
    torch = torch_cuda
    M, O, P = 8, 2, 3
    D = M // O
    taps = proto(X, M, P)
    other = np.abs(taps[::-1] * 2).astype(np.float32)
    rng = np.random.default_rng(8)
    n1, n2 = 5 * D + 1, 9 * D + 2
    raw = random_raw(rng, cm.FMT_C64, n1 + n2)
    x = raw.astype(np.complex128)
    ch = make(X, cm.FMT_C64, M, O, taps)
    a = ch.process(raw[:n1])
    ch.set_taps(other)                                             # the history is kept: the second piece sees the first through the new taps
    b = ch.process(raw[n1:])
    assert ch.state() == {"samples_in": n1 + n2, "samples_out": a.shape[1] + b.shape[1]}
    want_b = cm.polyphase(x, other, M, O)[:, a.shape[1]:]
    assert np.max(np.abs(b - want_b)) <= cm.bound(other, np.abs(raw).max(), M, P)
    ch.reset()
    assert ch.state() == {"samples_in": 0, "samples_out": 0}
    fresh = ch.process(raw[n1:])                                   # history and counts are gone
    want = cm.polyphase(x[n1:], other, M, O)
    assert np.max(np.abs(fresh - want)) <= cm.bound(other, np.abs(raw).max(), M, P)
    with pytest.raises(X.KsaError, match="set_taps"):
        ch.set_taps(taps[:-1])
    # set_stream orders old work first: the two halves of one stream on two torch streams equal one call
    ch.set_taps(taps)
    ch.reset()
    whole = ch.process(raw)
    ch.reset()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    keep, xd = to_dev(torch, raw)
    out = torch.zeros((M, whole.shape[1]), dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()
    ch.set_stream(s1.cuda_stream)
    c1 = ch.process_dev(xd, n1, out=out, chan_stride=whole.shape[1])
    ch.set_stream(s2.cuda_stream)
    c2 = ch.process_dev(xd[2 * n1:], n2, out=out[:, c1:], chan_stride=whole.shape[1])
    ch.synchronize()
    assert c1 + c2 == whole.shape[1] and np.array_equal(out.cpu().numpy(), whole)
    ch.set_stream(None)
    twin = make(X, cm.FMT_C64, M, O, other)                        # two objects of one shape share a kernel and do not share state
    t = twin.process(raw[n1:])
    assert np.array_equal(t, fresh) and twin.kernel_info() == {**ch.kernel_info(), "grid": twin.kernel_info()["grid"]}
    assert ch.state()["samples_in"] == n1 + n2 and twin.state()["samples_in"] == n2
    twin.close()
    ch.close()


def test_a_later_smaller_object_does_not_lower_the_lds_limit(X, torch_cuda):
    """The dynamic-LDS limit belongs to the kernel function, and every shape of one format runs the same chan_kernel, with 146 KiB
    at (1024, 4, 8) and 42 KiB at (16, 2, 8): the larger object, made first, still launches after the smaller one was made, and
    so does a second large one made after it."""
    torch = torch_cuda
    M, O, P = 1024, 4, 8
    taps = proto(X, M, P)
    big = make(X, cm.FMT_C64, M, O, taps)
    small = make(X, cm.FMT_C64, 16, 2, proto(X, 16, 8))
    assert big.kernel_info()["lds_bytes"] > 128 * 1024 and small.kernel_info()["lds_bytes"] < 64 * 1024
    n = (M // O) * 20 + 1
    raw = random_raw(np.random.default_rng(146), cm.FMT_C64, n)
    want = cm.polyphase(raw.astype(np.complex128), taps, M, O)
    b = cm.bound(taps, np.abs(raw).max(), M, P)
    assert small.process(raw[:100]).shape == (16, 13)
    got = run_stream(torch, big, raw, 0, n)
    assert got.shape == want.shape and np.max(np.abs(got - want)) <= b
    again = make(X, cm.FMT_C64, M, O, taps)
    assert np.array_equal(run_stream(torch, again, raw, 0, n), got)
    for obj in (again, small, big):
        obj.close()


def test_plan_is_a_function_of_the_shape(X, torch_cuda):
    for M, O, P in SHAPES:
        taps = proto(X, M, P)
        a = X.Channelizer(cm.FMT_C64, M, O, taps, max_in=64)
        b = X.Channelizer(cm.FMT_S8, M, O, taps, max_in=MAX_IN)
        ia, ib = a.kernel_info(), b.kernel_info()
        for k in ("threads", "lds_bytes", "tile_cols", "form"):
            assert ia[k] == ib[k], (M, O, P, k)
        assert ia["threads"] == cm.plan(M, O, P)[3] and ia["lds_bytes"] <= 160 * 1024 and ia["form"] == X.FORM_LDS
        W = ia["tile_cols"]
        assert (W, ia["lds_bytes"]) == (cm.plan(M, O, P)[0], cm.plan(M, O, P)[2])          # the rule DESIGN 4.16 writes down
        print("chan plan %s: W %d, threads %d, LDS %d bytes, VGPRs %d" % ((M, O, P), W, ia["threads"], ia["lds_bytes"], ia["vgprs"]))
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------ 9. the chain
def test_all_channels_into_the_demodulator_in_place(X, torch_cuda):
    """An FM signal in channel c0 and a weak unmodulated carrier at the centre of every other channel (so that every channel's
    phase is well conditioned), channelised with M = 16, O = 2; all 16 channels go through Demodulator.blocks_dev in one call
    that reads the channelizer's buffer in place.  An error e on a sample of magnitude A moves its phase by at most
    asin(e / A), an FM detector value (the difference of two phases) by twice that."""
    torch = torch_cuda
    demod = importlib.import_module("prgs-sdr-kspecanal_amd.demod")
    M, O, P, c0 = 16, 2, 8, 5
    D = M // O
    taps = proto(X, M, P)
    cols, dD = 1024, 4
    first = cm.first_column(M, O, P)
    n = D * (first + cols - 1) + 1
    tt = np.arange(n)
    offset, dev, fm = 0.004, 0.003, 1.0 / 128                     # cycles per input sample
    sig = 0.5 * np.exp(2j * np.pi * ((c0 / M + offset) * tt - dev / fm * np.cos(2 * np.pi * fm * tt) / (2 * np.pi)))
    for c in range(M):
        if c != c0:
            sig = sig + 0.02 * np.exp(2j * np.pi * (((c * tt) % M) / M + 0.001 * c * tt / M))
    raw = sig.astype(np.complex64)
    stream = torch.cuda.Stream()
    ch = X.Channelizer(cm.FMT_C64, M, O, taps, max_in=n, stream=stream.cuda_stream)
    dtaps = demod.demod_taps(dD, 8)
    dmo = demod.Demodulator("fm", dD, dtaps, max_in=M * cols, stream=stream.cuda_stream)
    keep, xd = to_dev(torch, raw)
    torch.cuda.synchronize()
    assert ch.process_dev(xd, n) == first + cols
    J = dmo.blocks_dev(ch.out_ptr + 8 * first, M, cols, block_stride=ch.out_stride)     # no synchronisation in between
    got = dmo.read_out(M * J).reshape(M, J)
    z = cm.polyphase(raw.astype(np.complex128), taps, M, O)[:, first:]
    want = mm.blocks(z, dtaps, dD, mm.MODE_FM)
    assert want.shape == (M, J)
    bc = cm.bound(taps, np.abs(raw).max(), M, P)
    sumd = np.abs(dtaps.astype(np.float64)).sum()
    for c in range(M):
        amin = np.abs(z[c]).min()
        assert amin > 100 * bc, (c, amin)
        tol = mm.bound(dtaps, mm.MODE_FM, np.abs(z[c]).max()) + sumd * 2 * np.arcsin(bc / amin) / (2 * np.pi)
        assert np.max(np.abs(got[c] - want[c])) <= tol, (c, np.max(np.abs(got[c] - want[c])), tol)
    # the mean of channel c0's FM output is the tone's offset, in turns per channel sample; what is left of the modulation
    # (amplitude dev * D turns, `periods` periods, the last one cut anywhere) is at most its amplitude / (pi * periods)
    periods = J * dD * D * fm
    left = dev * D / (np.pi * periods)
    assert abs(float(got[c0].mean()) - offset * D * float(dtaps.astype(np.float64).sum())) <= left + tol
    dmo.close()
    ch.close()


# ------------------------------------------------------------------------------------------ 10. command line
def test_cli_channels_end_to_end(tmp_path, capsys):
    K = importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")
    n, frames = 64, 6
    base = K.handle_args({}, ["zeroSpan", "fftSize", str(n), "channels", "8:2:4:3", "iqFormat", "s16", "frameBatch", "4", "demod", "fm:4:4"])
    c, fs, fc, full = base["chan.spec"], base["samplingRate"], base["centerFreq"], base["fullSize"]
    assert c["block_len"] == 4 * (8 + full - 1) + 1 and c["center"] == fc + 3 * fs / 8 and c["span"] == fs / 4
    settle = 16 * 1024                                 # the samples sdr_setup discards
    per_read = 1 << int(np.ceil(np.log2(c["block_len"])))
    t = np.arange(settle + frames * per_read)
    tone = 3 * fs / 8 + 5 * (fs / 4 / n)               # channel 3's centre plus five bins of the channel's spectrum
    rng = np.random.default_rng(10)
    x = 0.5 * np.exp(2j * np.pi * (tone / fs) * t) + 0.01 * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
    raw = np.empty(2 * t.size, dtype=np.int16)
    raw[0::2] = np.round(x.real * 32767)
    raw[1::2] = np.round(x.imag * 32767)
    path, save, wav = tmp_path / "cap_s16.bin", tmp_path / "levels.npz", tmp_path / "chan.wav"
    raw.tofile(path)
    common = ["zeroSpan", "fftSize", str(n), "iqFormat", "s16", "frameBatch", "4", "prgLoopCnt", str(frames), "source", "file:%s" % path,
              "bPltLevels", "false", "bPltHeatMap", "false"]
    K.sdr_curscan = K._gpu_curscan
    capsys.readouterr()
    d = K.main(common + ["channels", "8:2:4:3", "channelsSave", str(save), "demod", "fm:4:4", "demodSave", str(wav)])
    out = capsys.readouterr().out
    freqs = d["freqs"]
    assert len(freqs) == n and freqs[0] == c["center"] - fs / 8 and d["startFreq"] == c["center"] - fs / 8 and d["endFreq"] == c["center"] + fs / 8
    assert abs(freqs[int(np.argmax(d["Fft.Cur"]))] - (fc + tone)) <= fs / 4 / n
    assert "INFO: channels [8]" in out and "INFO:zero_span: channels [8]" in out and "strongest [3] at [%s] Hz" % (fc + 3 * fs / 8) in out
    z = np.load(save)
    assert z["power_db"].shape == (8,) and int(np.argmax(z["power_db"])) == 3 and int(np.argmax(d["channelsPower"])) == 3
    assert np.array_equal(z["freqs"], d["channelsFreqs"]) and z["freqs"][3] == fc + 3 * fs / 8
    assert (int(z["nchan"]), int(z["oversample"]), int(z["taps_per_branch"]), int(z["pick"]), int(z["values"])) == (8, 2, 4, 3, frames * full)
    chan = importlib.import_module("prgs-sdr-kspecanal_amd.chan")
    h = chan.chan_prototype(8, 4).astype(np.float64)
    gain = abs(np.sum(h * np.exp(-2j * np.pi * (5 * (fs / 4 / n) / fs) * np.arange(h.size))))      # the prototype at the tone's offset
    assert abs(z["power_db"][3] - 10 * np.log10(0.25 * gain ** 2)) < 0.05  # a tone of amplitude 0.5; the noise adds 2e-4 / 8
    # demod behind channels: the tone sits 5 bins above the channel's centre, which FM turns into a constant
    pcm = d["demodAudio"].astype(np.float64)
    assert d["demodRate"] == base["demod.spec"]["rate"] == int(round(fs / 16)) and pcm.size == frames * base["demod.spec"]["out_per_block"]
    assert abs(pcm.mean() / K.DEMOD_PCM_SCALE - 5.0 / n) < 1e-3
    with pytest.raises(SystemExit):
        K.main(common + ["channels", "8:2:4:3", "zoom", "4"])
    assert "exclude each other" in capsys.readouterr().out


def test_print_the_worst_float_ratios():
    for shape in SHAPES:
        if shape in WORST:
            print("chan worst error / bound %s: %.4f" % (shape, WORST[shape]))
