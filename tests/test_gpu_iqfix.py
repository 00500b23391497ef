"""The IQ corrector on the GPU against tests/iqfix_model.py.  Every comparison is np.array_equal: the sums are integers, the
output is four float32 operations per sample and the solve is float64 in a fixed order, so no tolerance exists."""
import importlib

import numpy as np
import pytest

import iqfix_model as qm
from conftest import load_pkg

pytestmark = pytest.mark.gpu

FMTS = ("c64", "u8", "s8", "s16")
PER_VEC = {"c64": 2, "u8": 8, "s8": 8, "s16": 4}
SENTINEL = -7.0
SOME = (0.0625, -0.03125, -0.125, 0.875)              # coefficients that are not the identity


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def X():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.iqfix")


@pytest.fixture(scope="module")
def capture():
    """The impaired s16 capture of the host tests at 4096 samples, its unpacked samples and its sums: made once, never changed."""
    raw = qm.impaired_capture(4096)
    xr, xi = qm.unpack(raw, "s16")
    return raw, xr, xi, qm.stats(xr, xi)


def samples(fmt, n, seed=5):
    """Raw samples [n] (complex64) or [n][2] (integers) that use the whole range of the format."""
    rng = np.random.default_rng(seed + n)
    if fmt == "c64":
        x = (0.7 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
        x[::7] *= np.float32(3.0)                      # some beyond +-4 in value or product
        return x
    info = np.iinfo(qm.DTYPES[fmt])
    return rng.integers(info.min, info.max + 1, size=(n, 2)).astype(qm.DTYPES[fmt])


def sample_bytes(raw):
    return 8 if raw.dtype == np.complex64 else 2 * raw.dtype.itemsize


def to_dev(torch, raw, offset=0):
    """(tensor that owns the memory, device address of the samples): `offset` samples into a 16-byte-aligned allocation."""
    raw = np.ascontiguousarray(raw)
    per = sample_bytes(raw)
    b = raw.view(np.uint8).reshape(-1)
    buf = torch.zeros(len(b) + per * offset + 16, dtype=torch.uint8, device="cuda")
    if len(b):
        buf[per * offset:per * offset + len(b)] = torch.from_numpy(b.copy())
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + per * offset


def out_buffer(torch, values, offset=0):
    """(tensor, address `offset` complex64 into it): float32 sentinels for `values` complex64 and three more."""
    t = torch.full((2 * (values + offset + 3),), SENTINEL, dtype=torch.float32, device="cuda")
    return t, t.data_ptr() + 8 * offset


def read_out(t, offset=0):
    return t.cpu().numpy()[2 * offset:].view(np.complex64)


def model_blocks(xr, xi, starts, length, coeffs):
    """(complex64 [nblocks][length] of model.apply, int64 [6] sums over the blocks as read)."""
    out = np.array([qm.apply(xr[s:s + length], xi[s:s + length], coeffs) for s in starts]).reshape(len(starts), length)
    sums = sum((qm.stats(xr[s:s + length], xi[s:s + length]) for s in starts), np.zeros(6, dtype=np.int64))
    return out, sums


# ------------------------------------------------------------------------------------------ sums and output against the model
@pytest.mark.parametrize("fmt", FMTS)
def test_sums_and_output_equal_the_model_at_every_length_and_alignment(X, torch_cuda, fmt):
    fix = X.IqCorrector(fmt=fmt, max_in=1 << 15)
    T, V = fix.kernel_info()["tile"], PER_VEC[fmt]
    assert T % V == 0 and T >= 256
    fix.set_coeffs(*SOME)
    for n in (0, 1, 2, V - 1, V, V + 1, T - 1, T, T + 1, 3 * T + 5):
        raw = samples(fmt, n)
        xr, xi = qm.unpack(raw, fmt)
        want, sums = qm.apply(xr, xi, SOME), qm.stats(xr, xi)
        for offset in (0, 1):                           # from a 16-byte boundary and from one sample behind it
            keep, ptr = to_dev(torch_cuda, raw, offset)
            out, optr = out_buffer(torch_cuda, n)
            fix.clear_stats()
            fix.blocks_dev(ptr if n else 0, 1, n, out=optr, accumulate=True)
            got = read_out(out)
            assert np.array_equal(got[:n], want), (fmt, n, offset)
            assert np.all(out.cpu().numpy()[2 * n:] == SENTINEL), (fmt, n, offset)     # nothing past the end
            assert np.array_equal(fix.read_stats(), sums), (fmt, n, offset)
    assert fix.kernel_info()["grid"] == 4 and fix.kernel_info()["threads"] == 256
    fix.close()


@pytest.mark.parametrize("fmt", FMTS)
def test_the_three_call_forms_agree_and_the_host_form_too(X, torch_cuda, fmt):
    fix = X.IqCorrector(fmt=fmt, max_in=1 << 15)
    T = fix.kernel_info()["tile"]
    n = 3 * T + 5
    raw = samples(fmt, n, seed=11)
    xr, xi = qm.unpack(raw, fmt)
    keep, ptr = to_dev(torch_cuda, raw, 1)
    fix.set_coeffs(*SOME)
    a, aptr = out_buffer(torch_cuda, n, 1)              # an output 8 bytes off the 16-byte grid
    b, bptr = out_buffer(torch_cuda, n)
    fix.blocks_dev(ptr, 1, n, out=aptr)                 # apply only
    assert np.array_equal(fix.read_stats(), np.zeros(6, dtype=np.int64))
    fix.accumulate_dev(ptr, 1, n)                       # accumulate only
    only = fix.read_stats()
    fix.clear_stats()
    fix.blocks_dev(ptr, 1, n, out=bptr, accumulate=True)   # both
    both = fix.read_stats()
    want = qm.apply(xr, xi, SOME)
    assert np.array_equal(read_out(a, 1)[:n], want) and np.array_equal(read_out(b)[:n], want)
    assert np.all(a.cpu().numpy()[:2] == SENTINEL) and np.all(a.cpu().numpy()[2 * (n + 1):] == SENTINEL)
    assert np.array_equal(only, both) and np.array_equal(both, qm.stats(xr, xi))
    # the host form, staged: the same output and the sums once more
    got = fix.apply(raw, accumulate=True)
    assert np.array_equal(got, want) and np.array_equal(fix.read_stats(), 2 * qm.stats(xr, xi))
    assert np.array_equal(fix.apply(raw), want) and fix.read_stats()[5] == 2 * n
    fix.close()


def test_identity_gives_the_unpacked_input_and_the_u8_parameters_are_used(X, torch_cuda):
    raw = samples("u8", 1000)
    fix = X.IqCorrector(fmt="u8", max_in=1000, u8_offset=100.0, u8_scale=50.0)
    xr, xi = qm.unpack(raw, "u8", 100.0, 50.0)
    assert np.array_equal(fix.apply(raw, accumulate=True), (xr + 1j * xi).astype(np.complex64))
    assert np.array_equal(fix.read_stats(), qm.stats(xr, xi))
    assert fix.get_coeffs() == dict(dc_i=0.0, dc_q=0.0, c=0.0, d=1.0, flags=0, mode=0, count=0)
    fix.close()
    raw = samples("c64", 777)
    fix = X.IqCorrector(fmt="c64", max_in=777)
    assert np.array_equal(fix.apply(raw), raw)
    fix.close()


def test_sums_add_across_calls_and_clear_zeroes_them(X, torch_cuda):
    fix = X.IqCorrector(fmt="s16", max_in=1 << 14)
    raw = samples("s16", 10000)
    xr, xi = qm.unpack(raw, "s16")
    keep, ptr = to_dev(torch_cuda, raw)
    total = np.zeros(6, dtype=np.int64)
    for at, n in ((0, 1), (1, 4999), (5000, 0), (5000, 4097), (9097, 903)):
        fix.accumulate_dev(ptr + 4 * at, 1, n)
        total += qm.stats(xr[at:at + n], xi[at:at + n])
        assert np.array_equal(fix.read_stats(), total)
    assert np.array_equal(total, qm.stats(xr, xi))      # however the input is cut into calls
    view = torch_cuda.as_tensor(fix.stats_view(), device="cuda")
    assert np.array_equal(view.cpu().numpy(), total)
    fix.clear_stats()
    assert np.array_equal(fix.read_stats(), np.zeros(6, dtype=np.int64))
    fix.accumulate_dev(ptr, 1, 3)
    assert np.array_equal(fix.read_stats(), qm.stats(xr[:3], xi[:3]))
    fix.close()


# ------------------------------------------------------------------------------------------ the block form
@pytest.mark.parametrize("fmt", ("c64", "u8", "s16"))
def test_block_form_strides_gaps_and_the_own_buffer(X, torch_cuda, fmt):
    nb, blen = 5, 4099                                  # more than a tile, no multiple of a vector
    fix = X.IqCorrector(fmt=fmt, max_in=nb * blen)
    raw = samples(fmt, nb * (blen + 9), seed=3)
    xr, xi = qm.unpack(raw, fmt)
    keep, ptr = to_dev(torch_cuda, raw)
    fix.set_coeffs(*SOME)
    for stride in (blen, blen + 9, blen - 100, 0):
        starts = [b * stride for b in range(nb)]
        want, sums = model_blocks(xr, xi, starts, blen, SOME)
        for out_stride in (blen, blen + 3):
            out, optr = out_buffer(torch_cuda, nb * out_stride)
            fix.clear_stats()
            fix.blocks_dev(ptr, nb, blen, block_stride=stride, out=optr, out_stride=out_stride, accumulate=True)
            got = read_out(out)[:nb * out_stride].reshape(nb, out_stride)
            assert np.array_equal(got[:, :blen], want), (fmt, stride, out_stride)
            assert np.all(got[:, blen:].view(np.float32) == SENTINEL)          # the gaps are untouched
            assert np.all(out.cpu().numpy()[2 * nb * out_stride:] == SENTINEL)
            assert np.array_equal(fix.read_stats(), sums), (fmt, stride)        # overlapped samples count twice
        fix.blocks_dev(ptr, nb, blen, block_stride=stride)                      # the library's own packed buffer
        own = torch_cuda.as_tensor(fix.out_view(nb * blen), device="cuda").cpu().numpy()
        assert np.array_equal(own.reshape(nb, blen), want), (fmt, stride)
    fix.close()


def test_complex64_in_place(X, torch_cuda):
    nb, blen, stride = 3, 4100, 4103
    fix = X.IqCorrector(fmt="c64", max_in=nb * blen)
    raw = samples("c64", nb * stride, seed=9)
    xr, xi = qm.unpack(raw, "c64")
    fix.set_coeffs(*SOME)
    for offset in (0, 1):
        keep, ptr = to_dev(torch_cuda, raw, offset)
        fix.clear_stats()
        fix.blocks_dev(ptr, nb, blen, block_stride=stride, out=ptr, out_stride=stride, accumulate=True)
        got = keep.cpu().numpy()[8 * offset:8 * offset + 8 * len(raw)].view(np.complex64).reshape(nb, stride)
        want, sums = model_blocks(xr, xi, [b * stride for b in range(nb)], blen, SOME)
        assert np.array_equal(got[:, :blen], want)
        assert np.array_equal(got[:, blen:], raw.reshape(nb, stride)[:, blen:])   # between the blocks the input stands
        assert np.array_equal(fix.read_stats(), sums)
    fix.close()


# ------------------------------------------------------------------------------------------ exactness
def test_ties_saturation_and_products_in_one_piece(X, torch_cuda):
    k = np.array([1, 3, 5, 7, -1, -3, -5, 2 ** 20 + 1, 2 ** 23 - 1], dtype=np.float64) * 2.0 ** -31
    xr = np.concatenate([k, [2.0 ** -15, 3 * 2.0 ** -16, -(2.0 ** -15)], [4, 5, -4, -7, 2, 3, 3, -3, 1e30, 0.5, 1.9999999]])
    xi = np.concatenate([k[::-1], [3 * 2.0 ** -16, 5 * 2.0 ** -15, 2.0 ** -16], [0, 0, 0, 0, 2, -3, 3, -3, -1e30, -0.25, 2.0000002]])
    # a product that a fused multiply-add would carry unrounded into the sum: c uI + d uQ with inexact products
    xr = np.concatenate([xr, [0.1, 0.3333333, 0.7]]).astype(np.float32)
    xi = np.concatenate([xi, [0.2, 0.1428571, -0.9]]).astype(np.float32)
    raw = (xr + 1j * xi).astype(np.complex64)
    fix = X.IqCorrector(fmt="c64", max_in=len(raw))
    coeffs = (np.float32(0.1), np.float32(-0.3), np.float32(1 / 3), np.float32(0.9))
    fix.set_coeffs(*coeffs)
    assert np.array_equal(fix.apply(raw, accumulate=True), qm.apply(xr, xi, coeffs))
    assert np.array_equal(fix.read_stats(), qm.stats(xr, xi))
    q = qm.quantities(xr, xi)
    assert list(q[0][:7]) == [0, 2, 2, 4, 0, -2, -2] and list(q[4][9:12]) == [2, 8, 0]      # the ties are in there
    fix.close()
    # s16 at -32768: the one value whose square is full scale
    raw = np.full((300, 2), -32768, dtype=np.int16)
    raw[::3, 1] = 32767
    fix = X.IqCorrector(fmt="s16", max_in=300)
    fix.apply(raw, accumulate=True)
    xr, xi = qm.unpack(raw, "s16")
    assert np.array_equal(fix.read_stats(), qm.stats(xr, xi)) and fix.read_stats()[2] == 300 * 2 ** 30
    fix.close()


# ------------------------------------------------------------------------------------------ the solve
def test_solve_equals_the_model_in_every_mode_and_corrects_with_it(X, torch_cuda, capture):
    raw, xr, xi, sums = capture
    fix = X.IqCorrector(fmt="s16", max_in=4096)
    fix.apply(raw, accumulate=True)
    assert np.array_equal(fix.read_stats(), sums)
    for mode, name in ((1, "dc"), (2, "iq"), (3, "dc+iq")):
        want = qm.solve(sums, mode)
        for m in (mode, name):
            got = fix.solve(m)
            assert got == {k: (float(v) if k in ("dc_i", "dc_q", "c", "d") else v) for k, v in want.items()}, (mode, got, want)
            assert all(np.float32(got[k]) == want[k] for k in ("dc_i", "dc_q", "c", "d")) and got["flags"] == 0 and got["count"] == 4096
        assert fix.get_coeffs() == got
        assert np.array_equal(fix.apply(raw), qm.apply(xr, xi, qm.coeffs_of(want))), mode
    image, dc = qm.rejections(fix.apply(raw))           # and it does what it is for
    assert image > 50 and dc > 45
    # the flags: a constant, and nothing at all
    fix.clear_stats()
    assert fix.solve(3) == dict(dc_i=0.0, dc_q=0.0, c=0.0, d=1.0, flags=X.FLAG_EMPTY, mode=3, count=0)
    fix.apply(np.full((64, 2), 8192, dtype=np.int16), accumulate=True)
    assert fix.solve("dc+iq") == dict(dc_i=0.25, dc_q=0.25, c=0.0, d=1.0, flags=X.FLAG_DEGENERATE, mode=3, count=64)
    # set and get
    fix.set_coeffs(0.5, -0.25, 0.125, 2.0)
    assert fix.get_coeffs() == dict(dc_i=0.5, dc_q=-0.25, c=0.125, d=2.0, flags=0, mode=0, count=0)
    fix.close()


def test_a_solve_does_not_change_work_already_enqueued(X, torch_cuda, capture):
    raw, xr, xi, sums = capture
    fix = X.IqCorrector(fmt="s16", max_in=4096)
    keep, ptr = to_dev(torch_cuda, raw)
    out, optr = out_buffer(torch_cuda, 4096)
    fix.set_coeffs(*SOME)
    fix.blocks_dev(ptr, 1, 4096, out=optr, accumulate=True)       # enqueue
    sol = fix.solve(3)                                             # solve: new coefficients from the sums of that very call
    assert np.array_equal(read_out(out)[:4096], qm.apply(xr, xi, SOME))         # read: the call kept the old ones
    want = qm.solve(sums, 3)
    assert all(np.float32(sol[k]) == want[k] for k in ("dc_i", "dc_q", "c", "d"))
    fix.blocks_dev(ptr, 1, 4096, out=optr)
    assert np.array_equal(read_out(out)[:4096], qm.apply(xr, xi, qm.coeffs_of(want)))
    fix.close()


# ------------------------------------------------------------------------------------------ large sums, the count limit
@pytest.fixture(scope="module")
def full_scale_block():
    rng = np.random.default_rng(2030)
    raw = rng.choice(np.array([-32768, 32767, -32767, 32766], dtype=np.int16), size=(1 << 14, 2))
    raw[::5] = rng.integers(-32768, 32768, size=(len(raw[::5]), 2)).astype(np.int16)
    return raw, qm.stats(*qm.unpack(raw, "s16"))


def test_large_sums_stay_integers_past_2_to_the_53(X, torch_cuda, full_scale_block):
    """One 64 KB block of 2^14 full-scale s16 samples read 2^14 times at block_stride 0, no output.  2^14 x 2^14 = 2^28 samples are
    one more than max_in allows in a call, so the 2^14 reads are two calls of 2^13 blocks; five odd samples go first so that the
    low bits of the sums are not zero."""
    raw, block = full_scale_block
    fix = X.IqCorrector(fmt="s16", max_in=1 << 27)
    keep, ptr = to_dev(torch_cuda, raw)
    fix.accumulate_dev(ptr, 1, 5)
    for _ in range(2):
        fix.accumulate_dev(ptr, 1 << 13, 1 << 14, block_stride=0)
    want = block * (1 << 14) + qm.stats(*qm.unpack(raw[:5], "s16"))
    got = fix.read_stats()
    assert np.array_equal(got, want)
    assert got[2] > 2 ** 53 and got[3] > 2 ** 53 and got[5] == 2 ** 28 + 5 and got[2] % (1 << 14) != 0
    assert fix.kernel_info()["grid"] > 1
    fix.close()


def test_count_limit_is_exact(X, torch_cuda, full_scale_block):
    raw, block = full_scale_block
    fix = X.IqCorrector(fmt="s16", max_in=1 << 27)
    keep, ptr = to_dev(torch_cuda, raw)
    for _ in range(8):
        fix.accumulate_dev(ptr, 1 << 13, 1 << 14, block_stride=0)
    want = block * (1 << 16)
    assert np.array_equal(fix.read_stats(), want) and want[5] == 2 ** 30
    out, optr = out_buffer(torch_cuda, 1)
    for call in (lambda: fix.accumulate_dev(ptr, 1, 1), lambda: fix.blocks_dev(ptr, 1, 1, out=optr, accumulate=True),
                 lambda: fix.apply(raw[:1], accumulate=True)):
        with pytest.raises(X.KsaError, match=r"would take the count of the sums from 1073741824 past 2\^30"):
            call()
    assert np.array_equal(fix.read_stats(), want) and np.all(out.cpu().numpy() == SENTINEL)
    fix.blocks_dev(ptr, 1, 1, out=optr)                 # without the sums the call is welcome
    fix.clear_stats()
    fix.accumulate_dev(ptr, 1, 1)
    assert fix.read_stats()[5] == 1
    fix.close()


# ------------------------------------------------------------------------------------------ refusals
def test_per_call_refusals_each_with_its_text_leave_the_object_as_it_was(X, torch_cuda, capture):
    raw, xr, xi, sums = capture
    fix = X.IqCorrector(fmt="s16", max_in=3000)
    keep, ptr = to_dev(torch_cuda, raw)
    out, optr = out_buffer(torch_cuda, 3000)
    fix.set_coeffs(*SOME)
    fix.accumulate_dev(ptr, 1, 1000)
    before, coeffs = fix.read_stats(), fix.get_coeffs()
    nan, inf = float("nan"), float("inf")
    cases = ((lambda: fix.blocks_dev(ptr, -1, 10), "nblocks -1 must be >= 0"),
             (lambda: fix.blocks_dev(ptr, 1, -10, block_stride=10), "block_len -10 must be >= 0"),
             (lambda: fix.blocks_dev(ptr, 1, 10, block_stride=-1), "block_stride -1 must be >= 0"),
             (lambda: fix.blocks_dev(ptr, 4, 1000), "4 blocks of 1000 samples exceed max_in 3000"),
             (lambda: fix.blocks_dev(ptr, 1, 3001), "1 blocks of 3001 samples exceed max_in 3000"),
             (lambda: fix.accumulate_dev(ptr, 2 ** 40, 2 ** 40), "blocks of 1099511627776 samples exceed max_in 3000"),
             (lambda: fix.blocks_dev(None, 1, 10), "null input pointer"),
             (lambda: fix.blocks_dev(ptr + 2, 1, 10), "input pointer is not aligned to the 4 bytes of a sample"),
             (lambda: fix.accumulate_dev(ptr + 1, 1, 10), "input pointer is not aligned"),
             (lambda: fix.accumulate_dev(None, 1, 10), "null input pointer"),
             (lambda: fix.accumulate_dev(ptr, 1, -1, block_stride=10), "block_len -1 must be >= 0"),
             (lambda: fix.blocks_dev(ptr, 2, 100, out=optr, out_stride=99), "out_stride 99 is shorter than the 100 samples of a block"),
             (lambda: fix.blocks_dev(ptr, 2, 100, out=optr + 4), "output pointer is not aligned to the 8 bytes"),
             (lambda: X.check(X.lib().kqf_apply(fix._h, None, 5, None, 1)), "null input pointer"),
             (lambda: X.check(X.lib().kqf_apply(fix._h, ptr, 5, None, 0)), "null output pointer"),
             (lambda: X.check(X.lib().kqf_apply(fix._h, ptr, -5, None, 0)), "n -5 must be >= 0"),
             (lambda: fix.apply(raw[:3001]), "n 3001 exceeds max_in 3000"),
             (lambda: fix.set_coeffs(nan, 0, 0, 1), "must be finite"), (lambda: fix.set_coeffs(0, inf, 0, 1), "must be finite"),
             (lambda: fix.set_coeffs(0, 0, -inf, 1), "must be finite"), (lambda: fix.set_coeffs(0, 0, 0, nan), "must be finite"),
             (lambda: fix.solve(0), "mode 0 is not"), (lambda: fix.solve(4), "mode 4 is not"), (lambda: fix.solve(7), "mode 7 is not"),
             (lambda: fix.solve(-1), "mode -1 is not"),
             (lambda: X.check(X.lib().kqf_get_coeffs(fix._h, None)), "null coefficients out pointer"),
             (lambda: X.check(X.lib().kqf_read_stats(fix._h, None)), "null sums pointer"),
             (lambda: X.check(X.lib().kqf_stats_dev(fix._h, None)), "null sums out pointer"),
             (lambda: X.check(X.lib().kqf_out_dev(fix._h, None)), "null out pointer"))
    for call, text in cases:
        with pytest.raises(X.KsaError) as e:
            call()
        assert text in str(e.value), (text, str(e.value))
        assert np.array_equal(fix.read_stats(), before) and fix.get_coeffs() == coeffs, text
    with pytest.raises(X.KsaError, match=r"unknown mode \[both\]"):
        fix.solve("both")
    assert np.all(out.cpu().numpy() == SENTINEL)
    fix.blocks_dev(0, 0, 10)                            # no-ops
    fix.blocks_dev(ptr, 3, 0, out=optr, out_stride=0)
    fix.accumulate_dev(0, 5, 0)
    assert np.array_equal(fix.read_stats(), before)
    fix.blocks_dev(ptr, 3, 1000, out=optr, accumulate=True)        # and the object still works
    assert fix.read_stats()[5] == 4000
    assert np.array_equal(read_out(out)[:3000], qm.apply(xr[:3000], xi[:3000], SOME))
    fix.close()


def test_set_stream_orders_the_work(X, torch_cuda, capture):
    raw, xr, xi, sums = capture
    fix = X.IqCorrector(fmt="s16", max_in=4096)
    keep, ptr = to_dev(torch_cuda, raw)
    s = torch_cuda.cuda.Stream()
    fix.accumulate_dev(ptr, 1, 2048)
    fix.set_stream(s.cuda_stream)
    fix.accumulate_dev(ptr + 4 * 2048, 1, 2048)
    assert np.array_equal(fix.read_stats(), sums)
    fix.set_stream(None)
    fix.synchronize()
    fix.close()


# ------------------------------------------------------------------------------------------ command line
def test_cli_iqfix_equals_the_classes_fed_the_model(ksa, X, torch_cuda, tmp_path, capsys):
    K = importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")
    sources = importlib.import_module("prgs-sdr-kspecanal_amd.sources")
    ddc = importlib.import_module("prgs-sdr-kspecanal_amd.ddc")
    n, frames, batch = 512, 8, 4
    zoom = "4:150000"
    settle = 16 * 1024                                  # the samples sdr_setup discards
    plain = K.handle_args({}, ["zeroSpan", "fftSize", str(n), "iqFormat", "s16", "frameBatch", str(batch)])
    zoomed = K.handle_args({}, ["zeroSpan", "fftSize", str(n), "iqFormat", "s16", "frameBatch", str(batch), "zoom", zoom])
    longest = zoomed["zoom.spec"]["block_len"]
    per_read = 1 << int(np.ceil(np.log2(longest)))
    cap = qm.impaired_capture(settle + frames * per_read, seed=7)
    path = tmp_path / "cap_s16.bin"
    cap.tofile(path)
    common = ["zeroSpan", "fftSize", str(n), "iqFormat", "s16", "frameBatch", str(batch), "prgLoopCnt", str(frames),
              "source", "file:%s" % path, "bPltLevels", "false", "bPltHeatMap", "false"]

    def blocks_of(block_len):
        src = sources.FileSdr(str(path), iq_format="s16")
        src.read_samples(settle)
        blocks = np.array([K.sdr_read(src, block_len, raw="s16") for _ in range(frames)])
        src.close()
        assert blocks.shape == (frames, 2 * block_len) and blocks.dtype == np.int16
        return blocks

    def engine(base):
        return ksa.SpectrumEngine(n, full_size=base["fullSize"], non_overlap=base["curScanNonOverlap"], window=base["theWin"],
                                  cumu_mode=base["curScanCumuMode"], gain=base["gain"], min_amp=base["minAmp4Clip"],
                                  xres=base["xRes"], max_frames=batch)

    def expect(base, blocks, block_len, track, mode=3):
        """(engine state, list of the model's solves) of the run fed model-corrected blocks."""
        eng = engine(base)
        z = base["zoom.spec"]
        dc = None
        if z is not None:
            dc = ddc.DownConverter(ksa.FMT_C64, z["decim"], ddc.ddc_lowpass(z["decim"], z["taps_per_phase"]), freq=z["offset"],
                                   sampling_rate=base["samplingRate"], max_in=batch * block_len)
        coeffs, solves = qm.IDENTITY, []
        for b in range(0, frames, batch):
            xr, xi = qm.unpack(blocks[b:b + batch].reshape(-1, 2), "s16")
            if not track and not solves:
                solves.append(qm.solve(qm.stats(xr, xi), mode))
                coeffs = qm.coeffs_of(solves[-1])
            fixed = qm.apply(xr, xi, coeffs)
            if track:
                solves.append(qm.solve(qm.stats(xr, xi), mode))
                coeffs = qm.coeffs_of(solves[-1])
            keep, ptr = to_dev(torch_cuda, fixed)
            if dc is not None:
                dc.blocks_dev(ptr, batch, block_len)
                eng.frames_dev(dc.out_ptr, ksa.FMT_C64, batch)
            else:
                eng.frames_dev(ptr, ksa.FMT_C64, batch)
            eng.synchronize()
        state = eng.state()
        eng.close()
        if dc is not None:
            dc.close()
        return state, solves

    def run(extra):
        K.sdr_curscan = K._gpu_curscan
        capsys.readouterr()
        d = K.main(common + extra)
        return d, capsys.readouterr().out

    def check(d, save, state, solves):
        for k in ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg", "fftHM"):
            assert np.array_equal(d[k], state[k]), k                            # bit for bit
        z = np.load(save)
        assert len(z["batch"]) == len(solves) and list(z["batch"]) == list(range(len(solves)))
        for i, sol in enumerate(solves):
            for k in ("dc_i", "dc_q", "c", "d"):
                assert z[k].dtype == np.float32 and z[k][i] == sol[k], (i, k)
            assert (z["flags"][i], z["count"][i]) == (sol["flags"], sol["count"])
            g, p = qm.imbalance_of(sol["c"], sol["d"])
            assert (z["gain_db"][i], z["phase_deg"][i]) == (g, p)
        for k in ("dc_i", "dc_q", "c", "d", "flags", "count", "sums", "gain_db", "phase_deg"):
            assert np.array_equal(d["iqfix"][k], z[k]), k
        return z

    full = plain["fullSize"]
    blocks = blocks_of(full)
    save = str(tmp_path / "iqfix.npz")
    # the first batch measured, every block corrected
    state, solves = expect(plain, blocks, full, track=False)
    d, out = run(["iqfix", "dc+iq", "iqfixSave", save])
    z = check(d, save, state, solves)
    assert np.array_equal(z["sums"][0], qm.stats(*qm.unpack(blocks[:batch].reshape(-1, 2), "s16"))) and z["count"][0] == batch * full
    assert (int(z["mode"]), bool(z["track"]), int(z["block_len"])) == (3, False, full)
    assert "INFO:zero_span: iqfix batches [2], solves [1]" in out
    raw_state, _ = run([])                              # the key off: another spectrum, with the spike and the image in it
    assert not np.array_equal(raw_state["Fft.Avg"], state["Fft.Avg"]) and raw_state["iqfix"] == ""
    # blocks=1: the first block alone is measured
    d, _ = run(["iqfix", "dc+iq:blocks=1", "iqfixSave", save])
    z = np.load(save)
    want = qm.solve(qm.stats(*qm.unpack(blocks[0].reshape(-1, 2), "s16")), 3)
    assert all(z[k][0] == want[k] for k in ("dc_i", "dc_q", "c", "d")) and z["count"][0] == full and int(z["blocks"]) == 1
    # behind it the zoom, fed the corrected blocks as complex64
    zlen = zoomed["zoom.spec"]["block_len"]
    zblocks = blocks_of(zlen)
    state, solves = expect(zoomed, zblocks, zlen, track=False)
    d, out = run(["zoom", zoom, "iqfix", "dc+iq", "iqfixSave", save])
    check(d, save, state, solves)
    assert "INFO: zoom [4]" in out
    # track: every batch is measured while it is corrected with what the batch before it solved to
    state, solves = expect(plain, blocks, full, track=True)
    d, out = run(["iqfix", "dc+iq:track", "iqfixSave", save])
    z = check(d, save, state, solves)
    assert len(solves) == 2 and bool(z["track"]) and "solves [2]" in out
    assert z["count"][1] == batch * full                # the sums were cleared between the batches
