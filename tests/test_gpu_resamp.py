"""The resampler on the GPU against tests/resamp_model.py (whose float32 emulation is checked against the bound on the CPU, in
tests/test_resamp_host.py).  Shapes (L, M, P) take both plans (1024 outputs per workgroup, four per thread; 256, one per
thread), the limits of T, of P and of the ratio, and one shape whose plan differs between real and complex samples.  Input
lengths sit on every edge of the loader and the tile: 1, 2, P-1, P, P+1, the input that yields one tile of outputs -1 / +1
sample, three tiles + 5, and once from a pointer one sample into a 16-byte-aligned allocation.  Exact inputs are compared with
np.array_equal, floats against the bound written down in resamp_model."""
import importlib
import subprocess
import sys
import wave

import numpy as np
import pytest

import resamp_model as rm
from conftest import ROOT, load_pkg

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 3, 4), (3, 1, 4), (2, 3, 5), (3, 2, 8), (147, 160, 12), (160, 147, 8), (1024, 1023, 8), (1024, 1, 16),
          (64, 1023, 256), (1, 16, 128), (1, 8, 16)]
# outputs per workgroup: 1024 where the span of 1024 outputs, ((1023 M + L - 1) div L + P) samples and one of padding per 32,
# stays within 40 KiB, else 256; (1, 8, 16) is 33.8 KiB of float32 and 67.7 KiB of complex64
SMALL = {(64, 1023, 256), (1, 16, 128)}
TYPES = ("f32", "c64")
WORST = {}                                   # (shape, type) -> worst error / bound of the float test, printed at the end


def tile_of(shape, typ):
    return 256 if shape in SMALL or (shape == (1, 8, 16) and typ == "c64") else 1024


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def X():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.resamp")


def need(m, L, M):
    """The shortest input that yields outputs 0 .. m."""
    return (m * M) // L + 1


def lengths_for(shape, t):
    """Input lengths on every edge of the loader and the tile."""
    L, M, P = shape
    tile = need(t - 1, L, M)
    return sorted({n for n in (1, 2, P - 1, P, P + 1, tile - 1, tile, tile + 1, need(3 * t + 4, L, M)) if n >= 1})


def max_in_for(shape, t):
    return max(need(3 * t + 4, *shape[:2]) + 8, 4 * shape[2] + 64)


def to_dev(torch, x, offset=0):
    """(tensor that owns the memory, device address of the samples): `offset` samples into a 16-byte-aligned allocation."""
    x = np.ascontiguousarray(x)
    per = 2 if x.dtype == np.complex64 else 1
    buf = torch.zeros(per * (len(x) + offset) + 4, dtype=torch.float32, device="cuda")
    if len(x):
        buf[per * offset:per * (offset + len(x))] = torch.from_numpy(x.view(np.float32))
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + 4 * per * offset


def fetch(torch, out, n, dtype):
    a = out.cpu().numpy()
    return a.view(np.complex64)[:n].copy() if dtype == np.complex64 else a[:n].copy()


def out_buffer(torch, rs, n):
    if rs.dtype == np.int16:
        return torch.zeros(max(n, 1), dtype=torch.int16, device="cuda")
    return torch.zeros(max(n, 1) * (2 if rs.dtype == np.complex64 else 1), dtype=torch.float32, device="cuda")


def run_stream(torch, rs, x, offset=0):
    """x through process_dev into a caller's buffer."""
    want = rs.out_count(len(x))
    out = out_buffer(torch, rs, want)
    keep, ptr = to_dev(torch, x, offset)
    got = rs.process_dev(ptr if len(x) else 0, len(x), out=out, out_capacity=want)
    assert got == want
    rs.synchronize()
    del keep
    return fetch(torch, out, got, rs.dtype)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def float_input(rng, n, typ):
    x = rng.uniform(-1, 1, n).astype(np.float32)
    return (x + 1j * rng.uniform(-1, 1, n)).astype(np.complex64) if typ == "c64" else x


def float_taps(rng, shape):
    L, M, P = shape
    return (rng.uniform(-1, 1, L * P) * np.hamming(L * P + 2)[1:-1]).astype(np.float32)


# ------------------------------------------------------------------------------------------ 1. impulse
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_impulse_places_every_tap_exactly(X, torch_cuda, shape):
    L, M, P = shape
    rng = np.random.default_rng(L * 100003 + M * 101 + P)
    taps = float_taps(rng, shape)
    for typ, fmt in (("f32", "same"), ("c64", "same"), ("f32", "s16")):
        t = tile_of(shape, typ)
        count = t + 2
        n_in = need(count - 1, L, M)
        assert rm.cdiv(n_in * L, M) >= count
        rs = X.Resampler(L, M, taps, type=typ, out_fmt=fmt, pcm_scale=1024.0, max_in=n_in)
        assert rs.kernel_info()["tile_out"] == t
        edge = need(t - 1, L, M) - 1                              # the newest sample of the tile's last output
        spots = {0, 1, 2, P - 1, P, P + 1, edge - P, edge - P + 1, edge - 1, edge, edge + 1, n_in - 1}
        m = np.arange(rm.cdiv(n_in * L, M))
        n, p = (m * M) // L, (m * M) % L
        c = np.complex64(1 - 2j) if typ == "c64" else np.float32(-2)
        for pos in sorted(s for s in spots if 0 <= s < n_in):
            x = np.zeros(n_in, dtype=rs.in_dtype)
            x[pos] = c
            rs.reset()
            y = rs.process(x)
            q = n - pos
            h = np.where((q >= 0) & (q < P), taps[p + np.clip(q, 0, P - 1) * L], np.float32(0)).astype(np.float32)
            want = (h * c.real + 1j * (h * c.imag)).astype(np.complex64) if typ == "c64" else h * c      # exact: times 1 or -2
            if fmt == "s16":
                want = rm.pcm(want, 1024.0)
            assert y.shape == want.shape and y.dtype == want.dtype and np.array_equal(y, want), (shape, typ, fmt, pos)
        rs.close()


# ------------------------------------------------------------------------------------------ 2. exact inputs
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_exact_inputs_in_every_type_format_and_form(X, torch_cuda, shape):
    torch = torch_cuda
    L, M, P = shape
    rng = np.random.default_rng(L * 7 + M * 13 + P)
    for typ, fmt, kind, scale in (("f32", "same", "int", 1.0), ("c64", "same", "pow2", 1.0), ("f32", "s16", "pow2", 0.25)):
        t = tile_of(shape, typ)
        taps, num, den = rm.exact_taps(rng, L * P, kind)
        out_fmt = rm.OUT_S16 if fmt == "s16" else rm.OUT_SAME
        bl_long = need(t, L, M) + P + 5                             # a block of more than one tile
        starts_len = 2 * (M + 1) + bl_long
        rs = X.Resampler(L, M, taps, type=typ, out_fmt=fmt, pcm_scale=scale, max_in=max(max_in_for(shape, t), 3 * bl_long))
        assert rs.kernel_info()["tile_out"] == t
        lengths = lengths_for(shape, t)
        for n in lengths:
            x = rm.exact_samples(rng, n, typ == "c64")
            rs.reset()
            got = run_stream(torch, rs, x, offset=1 if n == lengths[-1] or n == P else 0)
            want = rm.exact_stream(x, num, den, L, M, out_fmt, scale)
            assert got.dtype == want.dtype and np.array_equal(got, want), (shape, typ, fmt, n)
            assert rs.state() == {"samples_in": n, "samples_out": len(want)}
        # blocks: starts that are multiples of M (stride M) and starts that are not (stride M + 1); the model's own block definition
        x = rm.exact_samples(rng, starts_len, typ == "c64")
        keep, ptr = to_dev(torch, x, offset=1)
        before = rs.state()
        for stride, bl, own in ((M, bl_long, True), (M + 1, bl_long, False), (M + 1, P + rm.cdiv(M, L) + 3, False), (0, bl_long, True)):
            J = rm.block_out_count(bl, L, M, P)
            assert rs.block_out_count(bl) == J >= 1
            starts = [b * stride for b in range(3)]
            want = rm.exact_blocks(x, num, den, L, M, starts, bl, out_fmt, scale)
            if own:
                assert rs.blocks_dev(ptr, 3, bl, block_stride=stride) == J
                got = rs.read_out(3 * J).reshape(3, J)
            else:
                out = out_buffer(torch, rs, 3 * (J + 3))
                assert rs.blocks_dev(ptr, 3, bl, block_stride=stride, out=out, out_stride=J + 3) == J
                rs.synchronize()
                full = fetch(torch, out, 3 * (J + 3), rs.dtype).reshape(3, J + 3)
                got = full[:, :J]
                assert not np.any(full[:, J:])                     # nothing past a block's J outputs
            assert np.array_equal(got, want), (shape, typ, fmt, stride, bl)
            if stride == M:                                        # and those are the stream's outputs b L + first ...
                first = rm.block_first(L, M, P)
                whole = rm.exact_stream(x[:2 * M + bl], num, den, L, M, out_fmt, scale)
                for b in range(3):
                    assert np.array_equal(got[b], whole[b * L + first:b * L + first + J])
        assert rs.state() == before                                # the block form does not touch the stream
        rs.close()
        del keep


# ------------------------------------------------------------------------------------------ 3. floats inside the bound
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_floats_stay_inside_the_bound(X, torch_cuda, shape):
    torch = torch_cuda
    L, M, P = shape
    rng = np.random.default_rng(L * 31337 + M * 17 + P)
    taps = float_taps(rng, shape)
    for typ in TYPES:
        t = tile_of(shape, typ)
        n = need(3 * t + 4, L, M)
        x = float_input(rng, n, typ)
        rs = X.Resampler(L, M, taps, type=typ, max_in=n)
        got = run_stream(torch, rs, x)
        ms = np.arange(len(got))
        want = rm.at(x.astype(np.complex128 if typ == "c64" else np.float64), taps.astype(np.float64), L, M, ms)
        ratio = rm.worst_ratio(got, want, x, taps, L, M, ms)
        WORST[(shape, typ)] = ratio
        print("resampler float test %s %s: worst error / bound %.4f over %d outputs" % (shape, typ, ratio, len(got)))
        assert ratio <= 1.0, (shape, typ, ratio)
        rs.close()


def test_report_the_worst_ratio():
    print("resampler float test: worst error / bound per shape:", {k: round(v, 4) for k, v in WORST.items()})
    assert all(v <= 1.0 for v in WORST.values())


# ------------------------------------------------------------------------------------------ 4. cuts and blocks
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_the_cut_of_the_stream_does_not_show_and_blocks_are_the_stream(X, torch_cuda, shape):
    torch = torch_cuda
    L, M, P = shape
    rng = np.random.default_rng(L * 911 + M * 19 + P)
    taps = float_taps(rng, shape)
    for typ in TYPES:
        t = tile_of(shape, typ)
        n = need(3 * t + 4, L, M)
        x = float_input(rng, n, typ)
        rs = X.Resampler(L, M, taps, type=typ, max_in=4 * n + 64)      # room for three blocks of a third of it and their transients
        whole = run_stream(torch, rs, x)
        assert len(whole) == rm.cdiv(n * L, M)
        rs.reset()
        cuts = sorted(int(c) for c in rng.integers(0, n + 1, 7))
        cuts = [0, 0] + cuts[:3] + [cuts[2]] + cuts[3:] + [n, n]   # zero-length calls at the start, inside and at the end
        parts = [run_stream(torch, rs, x[a:b], offset=k % 2) for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:]))]
        assert np.array_equal(bits(np.concatenate(parts)), bits(whole)), (shape, typ, cuts)
        assert rs.state() == {"samples_in": n, "samples_out": len(whole)}
        # blocks that start k M samples into the stream
        first = rm.block_first(L, M, P)
        bl = min(n - 2 * M, need(t, L, M) + P + 5)
        if bl >= 1 and rm.block_out_count(bl, L, M, P) >= 1:
            keep, ptr = to_dev(torch, x)
            J = rs.blocks_dev(ptr, 3, bl, block_stride=M)
            got = rs.read_out(3 * J).reshape(3, J)
            for b in range(3):
                assert np.array_equal(bits(got[b]), bits(whole[b * L + first:b * L + first + J])), (shape, typ, b)
            del keep
        else:
            assert shape == (1024, 1, 16)                          # four samples in all: no block past its transient
        rs.close()


# ------------------------------------------------------------------------------------------ 5. positions past 32 bits in one call
def test_positions_past_32_bits_inside_one_call(X, torch_cuda):
    torch = torch_cuda
    L, M, P = 1024, 1023, 8
    rng = np.random.default_rng(2 ** 22 + 5)
    taps, num, den = rm.exact_taps(rng, L * P, "int")
    n = 2 ** 22 + 5
    x = rm.exact_samples(rng, n)
    rs = X.Resampler(L, M, taps, max_in=n)
    assert rs.kernel_info()["tile_out"] == 1024
    total = rm.cdiv(n * L, M)
    assert (total - 1) * M > 2 ** 32                               # t = m M leaves 32 bits inside this call
    keep, ptr = to_dev(torch, x)
    assert rs.process_dev(ptr, n) == total                         # into the object's own buffer
    m32 = 2 ** 32 // M
    for lo, hi in ((total - 4096, total), (max(0, m32 - 2048), min(total, m32 + 2048))):
        got = rs.read_out(hi - lo, first=lo)
        want = rm.exact_at(x, num, den, L, M, np.arange(lo, hi))
        assert np.array_equal(got, want), (lo, hi)
    assert rs.state() == {"samples_in": n, "samples_out": total}
    rs.close()
    del keep


# ------------------------------------------------------------------------------------------ 6. far stream positions
@pytest.mark.parametrize("shape", [(1024, 1023, 8), (147, 160, 12), (64, 1023, 256)], ids=str)
def test_far_stream_position(X, torch_cuda, shape):
    torch = torch_cuda
    L, M, P = shape
    rng = np.random.default_rng(40 + L)
    taps, num, den = rm.exact_taps(rng, L * P, "pow2")
    origin = 2 ** 40 + 12345
    rs = X.Resampler(L, M, taps, max_in=1 << 16)
    rs.reset_at(origin)
    m0 = rm.cdiv(origin * L, M)
    assert rs.state() == {"samples_in": origin, "samples_out": m0}
    at, m = origin, m0
    x = rm.exact_samples(rng, 3000)
    for a, b in ((0, 1), (1, 1), (1, 1700), (1700, 3000)):         # the history carries on across the calls
        k = rm.out_count(at, b - a, L, M)
        assert rs.out_count(b - a) == k
        got = run_stream(torch, rs, x[a:b])
        want = rm.exact_at(x[:b], num, den, L, M, [m + j for j in range(k)], origin)
        assert np.array_equal(got, want), (shape, a, b)
        at, m = at + (b - a), m + k
        assert rs.state() == {"samples_in": at, "samples_out": m}
    # the end of the permitted positions
    edge = X.MAX_POSITION - 10
    rs.reset_at(edge)
    state = rs.state()
    assert state == {"samples_in": edge, "samples_out": rm.cdiv(edge * L, M)}
    keep, ptr = to_dev(torch, x[:16])
    for call in (lambda: rs.process_dev(ptr, 11), lambda: rs.out_count(11), lambda: rs.process(x[:11])):
        with pytest.raises(X.KsaError, match="past 2\\^52"):
            call()
        assert rs.state() == state
    with pytest.raises(X.KsaError, match="samples_in"):
        rs.reset_at(X.MAX_POSITION + 1)
    with pytest.raises(X.KsaError, match="samples_in"):
        rs.reset_at(-1)
    assert rs.state() == state
    k = rm.out_count(edge, 10, L, M)
    got = run_stream(torch, rs, x[:10])
    assert np.array_equal(got, rm.exact_at(x[:10], num, den, L, M, [state["samples_out"] + j for j in range(k)], edge))
    assert rs.state() == {"samples_in": X.MAX_POSITION, "samples_out": rm.cdiv(X.MAX_POSITION * L, M)}
    rs.close()
    del keep


# ------------------------------------------------------------------------------------------ 7. refusals, taps, streams
def test_refusals_per_call_leave_the_object_as_it_was(X, torch_cuda):
    torch = torch_cuda
    L, M, P = 3, 2, 8
    rng = np.random.default_rng(99)
    taps = float_taps(rng, (L, M, P))
    rs = X.Resampler(L, M, taps, type="c64", max_in=4096)
    x = float_input(rng, 100, "c64")
    first = rs.process(x)
    keep, ptr = to_dev(torch, x)
    rs.blocks_dev(ptr, 2, 50)
    before, state = rs.read_out(rs.out_capacity), rs.state()
    small = torch.zeros(8, dtype=torch.float32, device="cuda")
    for call, text in ((lambda: rs.process_dev(0, 5), "null input pointer"),
                       (lambda: rs.process_dev(ptr + 4, 5), "not aligned"),
                       (lambda: rs.process_dev(ptr, -1), "n_in -1 must be >= 0"),
                       (lambda: rs.process_dev(ptr, 4097), "exceeds max_in"),
                       (lambda: rs.process_dev(ptr, 100, out=small, out_capacity=4), "output capacity 4 is too small"),
                       (lambda: rs.blocks_dev(0, 2, 50), "null input pointer"),
                       (lambda: rs.blocks_dev(ptr + 4, 2, 50), "not aligned"),
                       (lambda: rs.blocks_dev(ptr, -1, 50), "nblocks -1 must be >= 0"),
                       (lambda: rs.blocks_dev(ptr, 2, -50, block_stride=0), "block_len -50 must be >= 0"),
                       (lambda: rs.blocks_dev(ptr, 2, 50, block_stride=-1), "block_stride -1 must be >= 0"),
                       (lambda: rs.blocks_dev(ptr, 2, P - 1), "yields no output"),
                       (lambda: rs.blocks_dev(ptr, 100, 50), "exceed max_in"),
                       (lambda: rs.blocks_dev(ptr, 2, 50, out=small, out_stride=3), "out_stride 3 is shorter"),
                       (lambda: rs.read_out(5, first=-1), "first -1"), (lambda: rs.read_out(-5), "count -5"),
                       (lambda: rs.read_out(2, first=rs.out_capacity - 1), "outside the output buffer")):
        with pytest.raises(X.KsaError, match=text):
            call()
    assert not np.any(small.cpu().numpy())
    assert rs.block_out_count(P) == 1 and rs.blocks_dev(ptr, 0, P) == 1                   # the shortest block; no blocks: a no-op
    assert rs.process_dev(0, 0) == 0                       # n_in = 0 is a successful no-op, whatever the pointer
    assert rs.state() == state and np.array_equal(bits(rs.read_out(rs.out_capacity)), bits(before))
    tail = float_input(rng, 20, "c64")
    fresh = X.Resampler(L, M, taps, type="c64", max_in=4096)
    assert np.array_equal(bits(fresh.process(x)), bits(first))
    assert np.array_equal(bits(rs.process(tail)), bits(fresh.process(tail)))              # the history too
    # real samples are aligned to 4 bytes
    real = X.Resampler(L, M, taps, max_in=64)
    with pytest.raises(X.KsaError, match="not aligned to the 4 bytes"):
        real.process_dev(ptr + 2, 5)
    assert real.process_dev(ptr + 4, 5) == real.state()["samples_out"] == rm.cdiv(5 * L, M)
    for r in (fresh, rs, real):
        r.close()
    del keep


def test_set_taps_keeps_the_history(X, torch_cuda):
    rng = np.random.default_rng(7)
    L, M, P = 2, 3, 5
    a, b = float_taps(rng, (L, M, P)), float_taps(rng, (L, M, P))
    x = float_input(rng, 200, "f32")
    rs = X.Resampler(L, M, a, max_in=256)
    head = rs.process(x[:101])
    rs.set_taps(b)
    tail = rs.process(x[101:])
    ms = np.arange(len(head), rm.cdiv(200 * L, M))
    first = np.arange(len(head))
    assert len(head) == rm.cdiv(101 * L, M)
    assert rm.worst_ratio(head, rm.at(x.astype(np.float64), a.astype(np.float64), L, M, first), x, a, L, M, first) <= 1.0
    # every output after the switch is the new taps on the whole stream: the samples before the switch were kept
    assert len(tail) == len(ms)
    assert rm.worst_ratio(tail, rm.at(x.astype(np.float64), b.astype(np.float64), L, M, ms), x, b, L, M, ms) <= 1.0
    other = X.Resampler(L, M, b, max_in=256)
    assert np.array_equal(bits(other.process(x)[len(head):]), bits(tail))
    with pytest.raises(X.KsaError, match="set_taps wants"):
        rs.set_taps(b[:-1])
    bad = b.copy()
    bad[4] = np.nan
    with pytest.raises(X.KsaError, match="tap 4 is not finite"):
        rs.set_taps(bad)
    rs.close()
    other.close()


def test_set_stream_orders_the_work(X, torch_cuda):
    """The two halves of one stream on two torch streams equal one call: the second half needs the history that the first
    half's second launch writes."""
    torch = torch_cuda
    L, M = 147, 160
    rng = np.random.default_rng(8)
    taps = X.resample_taps(L, M, 6)
    P = len(taps) // L
    n = 1 << 18
    n1 = n // 2 + 3
    x = float_input(rng, n, "f32")
    keep, ptr = to_dev(torch, x)
    rs = X.Resampler(L, M, taps, max_in=n)
    assert rs.taps_per_phase == P == 12
    total = rs.out_count(n)
    out = torch.zeros(total, dtype=torch.float32, device="cuda")
    assert rs.process_dev(ptr, n, out=out, out_capacity=total) == total
    rs.synchronize()
    whole = out.cpu().numpy()
    assert rs.kernel_info()["grid"] == rm.cdiv(total, 1024)
    rs.reset()
    out.zero_()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    rs.set_stream(s1.cuda_stream)
    c1 = rs.process_dev(ptr, n1, out=out, out_capacity=total)
    rs.set_stream(s2.cuda_stream)
    c2 = rs.process_dev(ptr + 4 * n1, n - n1, out=out[c1:], out_capacity=total - c1)
    rs.synchronize()
    assert c1 + c2 == total and np.array_equal(bits(out.cpu().numpy()), bits(whole))
    rs.set_stream(None)
    info = rs.kernel_info()
    assert info["threads"] == 256 and info["tile_out"] == 1024 and 0 < info["vgprs"] <= 128 and 0 < info["lds_bytes"] <= 40 * 1024
    assert info["grid"] == rm.cdiv(c2, 1024)
    rs.close()
    del keep


# ------------------------------------------------------------------------------------------ 8. command line
def test_cli_resamples_the_audio_to_the_rate_asked_for(X, torch_cuda, tmp_path):
    torch = torch_cuda
    K = importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")
    ddc = importlib.import_module("prgs-sdr-kspecanal_amd.ddc")
    demod = importlib.import_module("prgs-sdr-kspecanal_amd.demod")
    fs, tone, dev, amp = 2048000.0, 1e3, 5e3, 0.5
    n_fft, frames = 256, 3
    args = ["zeroSpan", "fftSize", str(n_fft), "samplingRate", "2048000", "iqFormat", "s16", "zoom", "8", "demod", "fm:1"]
    base = K.handle_args({}, args + ["audioRate", "48000"])
    zs, ds, r = base["zoom.spec"], base["demod.spec"], base["resample.spec"]
    block_len, full = zs["block_len"], base["fullSize"]
    assert (ds["rate"], r["L"], r["M"]) == (256000, 3, 16) and block_len < 2 ** 18
    per_read = 1 << int(np.ceil(np.log2(block_len)))        # a block is one read, rounded up to a power of two and cut back
    settle = 16 * 1024                                      # what the set-up of the source reads and drops
    t = np.arange(settle + frames * per_read) / fs
    sig = amp * np.exp(1j * (dev / tone * np.sin(2 * np.pi * tone * t)))
    raw = np.empty(2 * t.size, dtype=np.int16)
    raw[0::2] = np.round(sig.real * 32767)
    raw[1::2] = np.round(sig.imag * 32767)
    path = tmp_path / "fm_s16.bin"
    raw.tofile(path)

    def run(extra, wav):
        p = subprocess.run([sys.executable, "-m", "prgs-sdr-kspecanal_amd.kspecanal"] + args + extra +
                           ["demodSave", str(wav), "source", "file:%s" % path, "prgLoopCnt", str(frames), "bPltLevels", "false",
                            "bPltHeatMap", "false"], capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        with wave.open(str(wav), "rb") as w:
            assert (w.getnchannels(), w.getsampwidth()) == (1, 2)
            return p.stdout, w.getframerate(), np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")

    out_on, rate_on, pcm_on = run(["audioRate", "48000"], tmp_path / "on.wav")
    out_off, rate_off, pcm_off = run([], tmp_path / "off.wav")
    J = r["out_per_block"]
    assert rate_on == 48000 and pcm_on.shape == (frames * J,)
    assert "INFO: audioRate [48000]: [256000] Hz -> [48000] Hz by L / M = [3] / [16]" in out_on and "at [48000] Hz, [%d] per block" % J in out_on
    assert rate_off == 256000 and pcm_off.shape == (frames * ds["out_per_block"],) and "audioRate" not in out_off

    # the same chain called directly: down-converter, demodulator, resampler
    blocks = np.stack([raw[2 * (settle + i * per_read):2 * (settle + i * per_read + block_len)] for i in range(frames)])
    dev_blocks = torch.from_numpy(blocks).to("cuda")
    dc = ddc.DownConverter(ddc.FMT_S16, zs["decim"], ddc.ddc_lowpass(zs["decim"], zs["taps_per_phase"]), freq=zs["offset"],
                           sampling_rate=fs, max_in=frames * block_len)
    assert dc.blocks_dev(dev_blocks, frames, block_len) == full
    taps = demod.demod_taps(ds["decim"], ds["taps_per_phase"])
    d32 = demod.Demodulator("fm", ds["decim"], taps, out_fmt="f32", max_in=frames * full)
    d16 = demod.Demodulator("fm", ds["decim"], taps, out_fmt="s16", pcm_scale=K.DEMOD_PCM_SCALE, max_in=frames * full)
    per = d32.blocks_dev(dc.out_ptr, frames, full)
    assert per == ds["out_per_block"] == d16.blocks_dev(dc.out_ptr, frames, full)
    assert np.array_equal(pcm_off, d16.read_out(frames * per))     # without the key: what the parent commit wrote
    rs = X.Resampler(r["L"], r["M"], X.resample_taps(r["L"], r["M"], r["taps_per_phase"]), out_fmt="s16", pcm_scale=K.DEMOD_PCM_SCALE,
                     max_in=frames * per)
    assert rs.blocks_dev(torch.as_tensor(d32.out, device="cuda"), frames, per) == J
    assert np.array_equal(pcm_on, rs.read_out(frames * J))
    # and it is the tone: its deviation in cycles per sample of the demodulator's rate, at the new rate
    want = dev / ds["rate"] * K.DEMOD_PCM_SCALE
    tt = np.arange(J) / 48000.0
    basis = np.stack([np.cos(2 * np.pi * tone * tt), np.sin(2 * np.pi * tone * tt)], axis=1)
    for b, y in enumerate(pcm_on.astype(np.float64).reshape(frames, J)):
        coef = np.linalg.lstsq(basis, y, rcond=None)[0]
        got = float(np.hypot(coef[0], coef[1]))
        print("resampler cli block %d: amplitude %.2f (want %.2f)" % (b, got, want))
        assert abs(got - want) <= 0.02 * want, (b, got, want)
    for o in (dc, d32, d16, rs):
        o.close()
