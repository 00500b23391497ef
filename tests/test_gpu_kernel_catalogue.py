"""One reference-checked GPU case per `recipe` of tests/kernel_catalogue.py: every templated kernel instantiation the
dispatchers of libksa.so and of the ten companions with templated kernels can select is launched once with the smallest input that can still go
wrong and compared with the float64 oracle or the library's own model.  That a case launches the kernel it names is measured
once by a kernel trace (tools/kernel_coverage.py, profiles/kernel_coverage.txt); here every case asserts what kernel_info()
shows of the selection (path, tile_out, form, threads).  kernel_info() cannot show that the pair kernel ran or whether a
launch was window-split: the pair rule (2 * grid frames and more, launch_spec_t) and the fill rule only size the batches, and
the trace is the proof.

Main library: five windows per frame (an odd count: a ragged round, and the odd tail of the ping-pong loop at 4096), three
frames at stride fullSize and, from N = 1024 up, a second batch of grid // 2 + 3 frames at stride 512 (the window-split and
the unsplit launch; at N = 1024, where `grid` is the pair kernel's, 2 * grid - 1 frames: the largest batch the pair kernel
does not take); the pair kernel takes 2 * grid + 1 frames at stride 64 (the rule of test_gpu_psd.py), the ring kernels
starts[k] == k * N; N >= 32768 runs two frames.  Companions: output counts t - 1, t, t + 1, 3 t + 7 around kernel_info()'s
tile, one call from a pointer that is not 16-byte aligned.

Tolerances are the project's own as they stand: assert_lin / assert_db / assert_psd, the models' exact equality for integers
and their `bound` for floats; the ring kernels are compared with the generic fold kernel bit for bit as well."""
import functools
import importlib

import numpy as np
import pytest

import chan_model as chm
import corr_model as cm
import ddc_model as dmod
import demod_model as mm
import density_model as dnm
import detect_model as dtm
import iqfix_model as qm
import kernel_catalogue as kc
import mask_model as mkm
import ksa_oracle as orc
import pfb_helper as pfb
import pfbpsd_helper as pp
import psd_helper as ph
import resamp_model as rm
import test_gpu_chan as tchan
import test_gpu_corr as tcorr
import test_gpu_ddc as tddc
import test_gpu_demod as tdemod
import test_gpu_density as tdensity
import test_gpu_detect as tdetect
import test_gpu_iqfix as tiqfix
import test_gpu_mask as tmask
import test_gpu_pulse as tpulse
import test_gpu_resamp as tresamp
from conftest import load_pkg
from test_gpu_parity import assert_lin
from test_gpu_pfb import SLICE
from test_gpu_psd import assert_psd

pytestmark = pytest.mark.gpu
CASES = kc.cases()
DIV = {2: 128.0, 3: 32768.0}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@functools.lru_cache(maxsize=4)
def stream(total, seed):
    return (orc.synth_iq(total, seed) * 0.6).astype(np.complex64)       # (shared between cases: nobody writes to it)


def in_format(x, fmt):
    """(the array handed to the device, the complex samples it stands for) of the complex64 stream x in format fmt."""
    if fmt == 0:
        return x, x
    if fmt == 1:
        raw = orc.quantize_u8(x)
        return raw, orc.unpack_u8(raw)
    top = 127 if fmt == 2 else 32767
    raw = np.empty(2 * len(x), dtype=np.int8 if fmt == 2 else np.int16)
    raw[0::2] = np.clip(np.round(x.real * top), -top - 1, top)
    raw[1::2] = np.clip(np.round(x.imag * top), -top - 1, top)
    return raw, (raw.astype(np.float32) / np.float32(DIV[fmt])).view(np.complex64)


def to_dev(torch, raw):
    raw = np.ascontiguousarray(raw)
    return (torch.view_as_real(torch.from_numpy(raw)) if raw.dtype == np.complex64 else torch.from_numpy(raw)).to("cuda")


def xres_for(n):
    return n if n <= 512 else 512 if n % 512 == 0 else 300 if n % 300 == 0 else 20


def expected_path(n):
    if n & (n - 1):
        return 6
    return 5 if n == 64 else 4 if n == 1024 else 3 if n in (8192, 16384) else 0 if n < 8192 else 2


def run_batches(torch, ksa, n, fmt, q, full, fold, window, batches, what):
    """An engine of five windows in fold mode `fold`; every (frames, stride) of `batches` (frames may be a function of
    kernel_info) through curscan_dev in format fmt, eight frames spread over the batch against the oracle.  Returns kernel_info."""
    win = orc.window_table(window, n)
    probe = ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window=window, cumu_mode=fold, xres=xres_for(n))
    info = probe.kernel_info()
    assert info["path"] == expected_path(n) and len(probe.starts) == 5, (what, info, probe.starts)
    probe.close()
    batches = [(f(info) if callable(f) else f, s) for f, s in batches]
    most = max(f for f, _ in batches)
    eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window=window, cumu_mode=fold, xres=xres_for(n), max_frames=most)
    for frames, stride in batches:
        x = stream((frames - 1) * stride + full, 1000 + n)
        raw, ref = in_format(x, fmt)
        out = torch.full((frames, n), -1.0, dtype=torch.float32, device="cuda")
        eng.curscan_dev(to_dev(torch, raw), fmt, frames, out, frame_stride=stride)
        eng.synchronize()
        got = out.cpu().numpy()
        assert np.all(got >= 0), what + ": a frame was not written"
        for f in sorted(set(np.linspace(0, frames - 1, min(frames, 8)).astype(int))):
            block = ref[f * stride:f * stride + full]
            tag = "%s frames %d stride %d frame %d" % (what, frames, stride, f)
            if fold == "PSD":
                assert_psd(got[f], ph.psd(block, n, q, win), what=tag)
            else:
                assert_lin(got[f], orc.curscan(block, n, q, win, fold), what=tag)
    eng.close()
    return info


def folds_of(cm_const):
    return ("AVG", "MAX", "MIN") if cm_const == 0 else (kc.FOLD_NAMES[cm_const],)


def geometry(n, rm):
    q, ratio = kc.HOPS[rm]
    return q, int(n * ratio)


# ---------------------------------------------------------------------------------------------- the main library
def case_spectrum(torch, ksa, n, fmt, rm, cm_const):
    q, full = geometry(n, rm)
    batches = [(3, full)]
    if n == 1024:        # `grid` is num_cu * pair_bpc there: the largest batch below the pair kernel's threshold (launch_spec_t)
        batches.append((lambda info: 2 * info["grid"] - 1, 512))
    elif n > 1024:
        batches.append((lambda info: info["grid"] // 2 + 3, 512))
    for fold in folds_of(cm_const):
        run_batches(torch, ksa, n, fmt, q, full, fold, "hanning", batches, "spectrum_kernel<%d, %d, %d, %d> %s" % (n, fmt, rm, cm_const, fold))


def case_pair(torch, ksa, fmt, rm, cm_const):
    q, full = geometry(1024, rm)
    # (path 4, asserted by run_batches: `grid` is num_cu * pair_bpc, and launch_spec_t pairs from 2 * grid frames up)
    run_batches(torch, ksa, 1024, fmt, q, full, kc.FOLD_NAMES[cm_const], "hamming", [(lambda info: 2 * info["grid"] + 1, 64)],
                "spectrum_pair_kernel<1024, %d, %d, %d>" % (fmt, rm, cm_const))


def case_spectrum32(torch, ksa, n, fmt, cm_const):
    q, full = geometry(n, 8)
    info = run_batches(torch, ksa, n, fmt, q, full, kc.FOLD_NAMES[cm_const], "kaiser", [(3, full), (lambda info: info["grid"] // 2 + 3, 512)],
                       "spectrum32_kernel<%d, %d, %d>" % (n, fmt, cm_const))
    assert info["path"] == 3


def case_spectrum64(torch, ksa, cm_const, w1):
    q, full = geometry(64, 0)
    info = run_batches(torch, ksa, 64, 0, q, full, kc.FOLD_NAMES[cm_const], "ones" if w1 else "hamming",
                       [(3, full), (lambda info: 2 * info["grid"] + 3, 64)], "spectrum64_kernel<0, %d, %s>" % (cm_const, w1))
    assert info["path"] == 5


def case_mr(torch, ksa, fmt, psd):
    for n in kc.MR_SIZES:
        for fold in (("PSD",) if psd else ("AVG", "MAX", "MIN")):
            info = run_batches(torch, ksa, n, fmt, 0.5, 3 * n, fold, "hamming", [(3, 3 * n), (1, 3 * n)], "mixed radix N=%d fmt %d %s" % (n, fmt, fold))
            assert info["path"] == 6


def case_dif(torch, ksa, n, fmt):
    q, full = geometry(n, 8)
    info = run_batches(torch, ksa, n, fmt, q, full, "AVG", "hanning", [(2, full)], "first stage N=%d fmt %d" % (n, fmt))
    assert info["path"] == 2


def pfb_engine(ksa, n, p, k, taps, frames):
    kw = dict(pfb_spectra=k) if k else {}
    return ksa.SpectrumEngine(n, pfb_taps=p, window=taps, xres=64, max_frames=frames, **kw)


def case_pfb_fold(torch, ksa, fmt):
    """P = 3 is no ring size: pfb_fold_kernel at stride N, against the model."""
    n, p, frames = 256, 3, 5
    taps = pfb.prototype(n, p, "hamming")
    raw, ref = in_format(stream((frames - 1 + p) * n, 31), fmt)
    eng = pfb_engine(ksa, n, p, 0, taps, frames)
    assert eng.kernel_info()["path"] == 0
    out = torch.full((frames, n), -1.0, dtype=torch.float32, device="cuda")
    eng.curscan_dev(to_dev(torch, raw), fmt, frames, out, frame_stride=n)
    eng.synchronize()
    got = out.cpu().numpy()
    for f in range(frames):
        assert_lin(got[f], pfb.spectrum(ref[f * n:(f + p) * n], n, taps), what="pfb_fold_kernel<%d> frame %d" % (fmt, f))
    eng.close()


def case_pfb_ring(torch, ksa, fmt, p):
    """Stride N (the ring kernel: starts[k] == k N, pfb_ring_pays) against the same frames as blocks at stride P N (the generic
    kernel) bit for bit, and against the model; 1, P - 1, P frames and three ring slices with an odd tail."""
    assert kc.pfb_ring_pays(fmt, p)
    n = 256
    counts = sorted({1, p - 1, p, 2 * SLICE + 3})
    most = counts[-1]
    taps = pfb.prototype(n, p, "hamming")
    raw, ref = in_format(stream((most - 1 + p) * n, 32 + p), fmt)
    per = 1 if fmt == 0 else 2
    blocks = np.stack([raw[f * n * per:(f + p) * n * per] for f in range(most)])
    eng = pfb_engine(ksa, n, p, 0, taps, most)
    assert np.array_equal(eng.starts, np.arange(p) * n)
    d_stream, d_blocks = to_dev(torch, raw), to_dev(torch, blocks.reshape(-1))
    for frames in counts:
        a = torch.full((frames, n), -1.0, dtype=torch.float32, device="cuda")
        b = torch.full((frames, n), -2.0, dtype=torch.float32, device="cuda")
        eng.curscan_dev(d_stream, fmt, frames, a, frame_stride=n)
        eng.curscan_dev(d_blocks, fmt, frames, b, frame_stride=p * n)
        eng.synchronize()
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert np.all(a >= 0) and np.array_equal(a, b), "pfb_ring_kernel<%d, %d> frames %d" % (fmt, p, frames)
        for f in sorted({0, frames - 1}):
            assert_lin(a[f], pfb.spectrum(ref[f * n:(f + p) * n], n, taps), what="pfb_ring_kernel<%d, %d> frame %d of %d" % (fmt, p, f, frames))
    eng.close()


def case_pfbpsd(torch, ksa, fmt, p, ring):
    """A P-tap block spectrometer against the model; the ring form (P in 4, 8, 16) also bit for bit against an engine of the
    same taps whose starts are all one N later (starts[0] != 0: never the ring form), fed the stream behind N more samples:
    the same samples, taps, K and scale through the generic form.  (test_gpu_pfbpsd.py's P + 1 taps do not reach P = 16.)"""
    n, k, blocks = 256, 2 * SLICE + 3, 3
    taps = pfb.prototype(n, p, "hamming")
    raw, ref = in_format(stream((blocks - 1) * k * n + (p + k) * n, 50 + p), fmt)
    a_eng = pfb_engine(ksa, n, p, k, taps, blocks)
    dev = to_dev(torch, raw)
    a = torch.full((blocks, n), -1.0, dtype=torch.float32, device="cuda")
    a_eng.curscan_dev(dev, fmt, blocks, a, frame_stride=k * n)
    a_eng.synchronize()
    a = a.cpu().numpy()
    assert np.all(a >= 0)
    for blk in range(blocks):
        assert_psd(a[blk], pp.spectrum(ref[blk * k * n:][:a_eng.full_size], n, taps), what="pfbpsd fmt %d P %d block %d" % (fmt, p, blk))
    if ring:
        assert kc.pfbpsd_ring_pays(fmt, p)
        b_eng = ksa.SpectrumEngine(n, pfb_taps=p, pfb_spectra=k, window=taps, xres=64, max_frames=blocks,
                                   starts=(np.arange(p) + 1) * n, full_size=a_eng.full_size + n)
        assert b_eng.mag_scale == a_eng.mag_scale and b_eng.pfb_spectra == k
        b = torch.full((blocks, n), -2.0, dtype=torch.float32, device="cuda")
        shifted = to_dev(torch, np.concatenate([np.zeros(n * (1 if fmt == 0 else 2), dtype=raw.dtype), raw]))
        b_eng.curscan_dev(shifted, fmt, blocks, b, frame_stride=k * n)
        b_eng.synchronize()
        assert np.array_equal(a, b.cpu().numpy()), "pfbpsd_ring_kernel<%d, %d> against the generic form" % (fmt, p)
        b_eng.close()
    a_eng.close()


# ---------------------------------------------------------------------------------------------- the companions
def counts_around(t):
    return [t - 1, t, t + 1, 3 * t + 7] if t > 1 else [1, 2, 10]


def dev_stream(torch, raw, offset):
    """(owner, tensor view) of raw on the device, `offset` samples into a 16-byte-aligned allocation."""
    per = 1 if raw.dtype == np.complex64 else 2
    pad = np.zeros(per * offset, dtype=raw.dtype)
    whole = to_dev(torch, np.concatenate([pad, raw]))
    assert whole.data_ptr() % 16 == 0
    view = whole[offset:] if raw.dtype == np.complex64 else whole[per * offset:]
    return whole, view


def ddc_run(torch, dc, raw, n_in, offset=0, first=0):
    per = 1 if raw.dtype == np.complex64 else 2
    want = dc.out_count(n_in)
    out = torch.zeros(max(want, 1), dtype=torch.complex64, device="cuda")
    keep, view = dev_stream(torch, raw[per * first:per * (first + n_in)], offset)
    if offset:
        assert view.data_ptr() % 16 != 0
    assert dc.process_dev(view, n_in, out=out, out_capacity=want) == want
    dc.synchronize()
    del keep
    return out[:want].cpu().numpy()


def case_ddc(torch, X, fmt, r):
    D, T = kc.DDC_SHAPES[r]
    rng = np.random.default_rng(9000 + 10 * fmt + D)
    want_plan = (8, 1) if r == "reduce" else (256 * r, 0)
    kw = dict(u8_offset=128.0, u8_scale=128.0) if fmt == dmod.FMT_U8 else {}
    # integers, exact (every partial sum a float32 value), the tile forms; the stream cut in two: the history kernel's rows
    if r != "reduce":
        taps = rng.integers(-8, 9, T)
        taps[0], taps[-1] = 8, -7
        amp = min(2 ** 23 // int(np.abs(taps).sum()), {0: 32767, 1: 127, 2: 127, 3: 32767}[fmt])
        dc = X.DownConverter(fmt, D, taps.astype(np.float32), phase_inc=2 ** 62, max_in=1 << 18, **kw)
        info = dc.kernel_info()
        assert (info["tile_out"], info["form"]) == want_plan and info["threads"] == 256, info
        for i, count in enumerate(counts_around(info["tile_out"])):
            n_in = D * (count - 1) + 1
            raw = tddc.int_raw(rng, fmt, n_in, amp)
            iq, scale = dmod.to_int(raw, fmt)
            want = dmod.int_stream(iq, scale, taps, D, dmod.phases(n_in, 2 ** 62))
            dc.reset()
            assert np.array_equal(ddc_run(torch, dc, raw, n_in, offset=1 if i == 2 else 0), want), (fmt, r, count)
            cut = n_in // 2 + 1
            dc.reset()
            pieces = np.concatenate([ddc_run(torch, dc, raw, cut), ddc_run(torch, dc, raw, n_in - cut, first=cut, offset=1)])
            assert np.array_equal(pieces, want), (fmt, r, count, "cut")
        dc.close()
    # floats inside the model's bound, every form
    taps = tddc.lowpass(X, D, T)
    dc = X.DownConverter(fmt, D, taps, phase_inc=tddc.INC, max_in=1 << 18)
    info = dc.kernel_info()
    assert (info["tile_out"], info["form"]) == want_plan, info
    for i, count in enumerate(counts_around(info["tile_out"])):
        n_in = D * (count - 1) + 1
        raw = tddc.random_raw(rng, fmt, n_in)
        x = dmod.unpack(raw, fmt)
        want = dmod.fir_at(x * dmod.rotor(dmod.phases(n_in, tddc.INC)), taps, D, 0, count)
        dc.reset()
        got = ddc_run(torch, dc, raw, n_in, offset=1 if i == 2 else 0)
        limit = dmod.bound(taps, np.abs(x).max())
        worst = float(np.max(np.abs(got.astype(np.complex128) - want))) / limit
        assert got.shape == want.shape and worst <= 1.0, (fmt, r, count, worst)
    dc.close()


def case_corr(torch, X, q):
    shape, G = (kc.CORR_K, q), 5
    K = kc.CORR_K
    W = tcorr.tile_of(shape)
    full = 3 * W + 7 + K - 1
    c, x = tcorr.exact_stream(shape, G, full)
    rho_all, r_all = cm.exact_model(x, c)
    cr = X.Correlator(c, threshold=0.5, guard=G, capacity=1 << 16, max_in=full + 8)
    info = cr.kernel_info()
    assert info["tile_out"] == W == (2048 if q <= 2 else 1024) and info["threads"] == 256, info
    for lags in (W - 1, W, W + 1, 3 * W + 7):
        cr.reset()
        rho, r, ev, total = tcorr.run_stream(torch, cr, x[:lags + K - 1], offset=1 if lags == W + 1 else 0)
        assert np.array_equal(rho, rho_all[:, :lags]) and np.array_equal(r, r_all[:, :lags]), (q, lags)
        want = cm.records(rho_all[:, :lags], r_all[:, :lags], 0.5, G)
        assert total == len(want) and tcorr.events_equal(ev, want), (q, lags)
    cr.close()
    # floats inside the model's bound
    rng = np.random.default_rng(700 + q)
    cf = (rng.uniform(-1, 1, (q, K)) + 1j * rng.uniform(-1, 1, (q, K))).astype(np.complex64)
    xf = tcorr.rand_c64(rng, W + 1 + K - 1)
    cr = X.Correlator(cf, threshold=1.0, guard=1, max_in=len(xf))
    rho, r, _, _ = tcorr.run_stream(torch, cr, xf)
    cr.close()
    w_rho, w_r = cm.worst_ratios(rho, r, xf, cf)
    assert w_rho <= 1.0 and w_r <= 1.0, (q, w_rho, w_r)


def case_chan(torch, X, fmt):
    """chan_kernel<fmt> and history_kernel<fmt>: integers exactly on the axis channels, the stream whole and cut in two (the second
    call reads the rows history_kernel wrote after the first), the second piece from an unaligned pointer; floats inside the bound."""
    M, O, P = kc.CHAN_SHAPE
    T, D = M * P, M // O
    rng = np.random.default_rng(8100 + fmt)
    taps = rng.integers(-3, 4, T)
    taps[0], taps[-1] = 2, -3
    ch = tchan.make(X, fmt, M, O, taps.astype(np.float32))
    info = ch.kernel_info()
    W = info["tile_cols"]
    assert ch.decim == D and ch.ntaps == T and W >= 1, info
    chans = (0, M // 4, M // 2, 3 * M // 4)
    for i, cols in enumerate(counts_around(W)):
        n = D * (cols - 1) + 1
        raw = tchan.int_raw(rng, fmt, n, min(100, 2 ** 23 // (3 * T)))
        iq, scale = chm.to_int(raw, fmt)
        want = {c: chm.int_channel(iq, scale, taps, M, O, c, np.arange(cols)) for c in chans}
        ch.reset()
        y = tchan.run_stream(torch, ch, raw, 0, n, lead=1 if i == 2 else 0)
        assert y.shape == (M, cols) and all(np.array_equal(y[c], want[c]) for c in chans), (fmt, cols)
        cut = n // 2 + 1
        ch.reset()
        y = np.concatenate([tchan.run_stream(torch, ch, raw, 0, cut), tchan.run_stream(torch, ch, raw, cut, n - cut, lead=1)], axis=1)
        assert y.shape == (M, cols) and all(np.array_equal(y[c], want[c]) for c in chans), (fmt, cols, "cut")
    ch.close()
    ftaps = tchan.proto(X, M, P)
    ch = tchan.make(X, fmt, M, O, ftaps)
    n = D * (3 * W + 6) + 1
    raw = tchan.random_raw(rng, fmt, n)
    x = tchan.unpacked(raw, fmt)
    cut = n // 2 + 1
    y = np.concatenate([tchan.run_stream(torch, ch, raw, 0, cut, lead=1), tchan.run_stream(torch, ch, raw, cut, n - cut)], axis=1)
    want = chm.polyphase(x, ftaps, M, O)
    assert y.shape == want.shape and float(np.max(np.abs(y - want)) / chm.bound(ftaps, np.abs(x).max(), M, P)) <= 1.0, fmt
    ch.close()


def case_demod(torch, X, mode, r, out):
    """tile_kernel<mode, r, out> and history_kernel<mode>: the model's exact inputs, whole and cut in two (FM also needs the
    last sample of the first piece)."""
    D, T = kc.DEMOD_SHAPES[r]
    t = 1024 if r == 4 else 256
    mode = tdemod.MODES[mode]
    fmt, name = (mm.OUT_F32, "f32") if out == "float" else (mm.OUT_S16, "s16")
    rng = np.random.default_rng(8200 + 10 * mode + r)
    taps = rng.integers(-8, 9, T).astype(np.float64)
    taps[0], taps[-1], taps[1], taps[2] = 8, -7, 0.5, -0.25
    counts = counts_around(t)
    longest = D * (counts[-1] - 1) + 1
    x, dn, dden, _ = tdemod.exact_input(rng, longest + 1, mode)
    conv = mm.exact_conv(dn, dden, taps)
    y = np.abs(mm.exact_stream(dn[:longest], dden, taps, D, conv=conv).astype(np.float64))
    pcm_scale = 2.0 ** np.ceil(np.log2(32768 / np.median(y[y > 0])))
    dm = X.Demodulator(tdemod.NAMES[mode], D, taps, out_fmt=name, pcm_scale=pcm_scale, max_in=1 << 18)
    assert dm.kernel_info()["tile_out"] == t, dm.kernel_info()
    for i, count in enumerate(counts):
        n = D * (count - 1) + 1
        want = mm.exact_stream(dn[:n], dden, taps, D, fmt, pcm_scale, conv=conv)
        dm.reset()
        got = tdemod.run_stream(torch, dm, x[:n], 1 if i == 2 else 0)
        assert len(want) == count and got.dtype == want.dtype and np.array_equal(got, want), (mode, r, out, count)
        cut = n // 2 + 1
        dm.reset()
        got = np.concatenate([tdemod.run_stream(torch, dm, x[:cut]), tdemod.run_stream(torch, dm, x[cut:n], 1)])
        assert np.array_equal(got, want), (mode, r, out, count, "cut")
    dm.close()


def case_resamp(torch, X, typ, r, fmt):
    """tile_kernel<element, r, output> and history_kernel<element>: the model's exact inputs, whole and cut in two."""
    L, M, P = kc.RESAMP_SHAPES[r]
    t = 1024 if r == 4 else 256
    kind, scale = {("f32", "same"): ("int", 1.0), ("c64", "same"): ("pow2", 1.0), ("f32", "s16"): ("pow2", 0.25)}[(typ, fmt)]
    rng = np.random.default_rng(8300 + r + len(typ + fmt))
    taps, num, den = rm.exact_taps(rng, L * P, kind)
    out_fmt = rm.OUT_S16 if fmt == "s16" else rm.OUT_SAME
    counts = counts_around(t)
    rs = X.Resampler(L, M, taps, type=typ, out_fmt=fmt, pcm_scale=scale, max_in=tresamp.need(counts[-1], L, M) + 8)
    assert rs.kernel_info()["tile_out"] == t, rs.kernel_info()
    for i, count in enumerate(counts):
        n = tresamp.need(count - 1, L, M)
        x = rm.exact_samples(rng, n, typ == "c64")
        want = rm.exact_stream(x, num, den, L, M, out_fmt, scale)
        assert len(want) >= count
        rs.reset()
        got = tresamp.run_stream(torch, rs, x, offset=1 if i == 2 else 0)
        assert got.dtype == want.dtype and np.array_equal(got, want), (typ, r, fmt, count)
        cut = n // 2 + 1
        rs.reset()
        got = np.concatenate([tresamp.run_stream(torch, rs, x[:cut]), tresamp.run_stream(torch, rs, x[cut:], offset=1)])
        assert np.array_equal(got, want), (typ, r, fmt, count, "cut")
    rs.close()


def case_pulse(torch, X, fmt):
    """env_kernel, both runs_kernel passes and hist_kernel of one format: the envelope and the pulse list against the model, the
    stream whole and cut in two (the second call's envelope reads the history the first left)."""
    name = kc.FMT_NAMES[fmt]
    kw = dict(u8_offset=127.4, u8_scale=127.6) if name == "u8" else {}
    det = X.PulseDetector(W=7, on_power=0.05, off_power=0.02, capacity=4096, max_in=1 << 14, fmt=name, **kw)
    T = det.kernel_info()["tile"]
    assert 3 * T + 7 <= 1 << 14
    rng = np.random.default_rng(8400 + fmt)
    found = 0
    for i, n in enumerate(counts_around(T)):
        s16 = tpulse.bursty_s16(rng, n)
        raw = {"c64": ((s16[:, 0] + 1j * s16[:, 1]) / 32768.0 * 1.7).astype(np.complex64), "u8": np.clip(s16 // 128 + 128, 0, 255).astype(np.uint8),
               "s8": (s16 // 256).astype(np.int8), "s16": s16}[name]
        det.reset()
        found += len(tpulse.check_against_model(tpulse.run_stream(torch, det, raw, offset=1 if i == 2 else 0), raw, 7, 0.05, 0.02, fmt=name, **kw))
        det.reset()
        cut = n // 2 + 1
        tpulse.check_against_model(tpulse.run_stream(torch, det, raw, pieces=[cut, n - cut], offset=1), raw, 7, 0.05, 0.02, fmt=name, **kw)
    assert found > 5
    det.close()


def case_iqfix(torch, X, fmt, apply, acc):
    """fix_kernel<fmt, apply, acc>: the corrected samples and / or the six sums against the model, exactly."""
    name = kc.FMT_NAMES[fmt]
    fix = X.IqCorrector(fmt=name, max_in=1 << 15)
    info = fix.kernel_info()
    T = info["tile"]
    assert T % tiqfix.PER_VEC[name] == 0 and info["threads"] == 256, info
    fix.set_coeffs(*tiqfix.SOME)
    for i, n in enumerate(counts_around(T)):
        raw = tiqfix.samples(name, n, seed=40 + fmt)
        xr, xi = qm.unpack(raw, name)
        keep, ptr = tiqfix.to_dev(torch, raw, 1 if i == 2 else 0)
        fix.clear_stats()
        if apply:
            out, optr = tiqfix.out_buffer(torch, n)
            fix.blocks_dev(ptr, 1, n, out=optr, accumulate=acc)
            assert np.array_equal(tiqfix.read_out(out)[:n], qm.apply(xr, xi, tiqfix.SOME)), (fmt, apply, acc, n)
            assert np.all(out.cpu().numpy()[2 * n:] == tiqfix.SENTINEL)
        else:
            fix.accumulate_dev(ptr, 1, n)
        want = qm.stats(xr, xi) if acc else np.zeros(6, dtype=np.int64)
        assert np.array_equal(fix.read_stats(), want), (fmt, apply, acc, n)
    fix.close()


def padded_rows(torch, rows, vec, fill):
    """(device view, row stride): the rows as they are from an aligned allocation (the 16-byte form), or one float into it at a
    stride of nbins + 3 with `fill` between the rows (the 4-byte form)."""
    nrows, nbins = rows.shape
    if vec:
        dev = torch.from_numpy(np.array(rows)).cuda()
        assert dev.data_ptr() % 16 == 0 and nbins % 4 == 0
        return dev, nbins
    stride = nbins + 3
    padded = np.full(1 + nrows * stride, fill, dtype=np.float32)
    padded[1:].reshape(nrows, stride)[:, :nbins] = rows
    dev = torch.from_numpy(padded).cuda()[1:]
    assert dev.data_ptr() % 16 == 4
    return dev, stride


def case_density(torch, X, vec, combine):
    """add_kernel<vec, combine>: the histogram of one call against the model, exactly; `combine`: four bins share a column."""
    nbins, levels = 64, 256
    width = 16 if combine else 64
    lo, hi = tdensity.RANGE[levels]
    for nrows in (1, 3, 257):
        rows = tdensity.cloud(9100 + nrows, nrows, nbins, levels, lo, hi)
        dev, stride = padded_rows(torch, rows, vec, np.nan)
        dens = X.SpectrumDensity(nbins, width, levels, lo, hi)
        dens.add_rows_dev(dev, nrows, row_stride=stride)
        got, seen = dens.read()
        info = dens.kernel_info()
        dens.close()
        assert seen == nrows and info["threads"] == 256 and np.array_equal(got, dnm.histogram(rows, width, levels, lo, hi)), (vec, combine, nrows)


def case_detect(torch, X, vec):
    """row_kernel<vec, false> and <vec, true> (both passes of one call): row counts, hits, emissions and the floor line against
    the model; row counts either side of a workgroup's rows."""
    nbins, cfg = 64, (8, 1, "ca", 1, 2)
    per = tdetect.rows_per_wg(nbins)
    for nrows in counts_around(per):
        rows = tdetect.cloud(9200 + nrows, nrows, nbins)
        want = dtm.detect(rows, 8, 1, tdetect.THRESHOLD, "ca", 1, 2, capacity=1 << 20)
        dev, stride = padded_rows(torch, rows, vec, np.float32(40.0))
        got = tdetect.run_dev(X, torch, dev, nrows, nbins, cfg, row_stride=stride)
        assert got["info"]["vec"] == int(vec) and got["info"]["rows_per_wg"] == per and got["info"]["threads"] == 256, got["info"]
        tdetect.assert_same(got, want, nrows)
    assert want["total"] > 0


def case_mask(torch, X, vec):
    """check_kernel<vec>: hits, events and row flags against the model."""
    nbins = 64
    up, lo = tmask.lines_for(nbins, True)
    for nrows in (2, 37, 257):
        rows = tmask.cloud(9300 + nrows, nrows, nbins, up, lo)
        want = mkm.check(rows, up, lo, 1)
        assert want["event"].any() and not want["event"].all()
        dev, stride = padded_rows(torch, rows, vec, np.nan)
        flag = torch.zeros(nrows, dtype=torch.uint8, device="cuda")
        m = X.SpectrumMask(nbins, up, lo)
        m.check_rows_dev(dev, nrows, row_stride=stride, row_event=flag)
        got = m.hits() + m.events() + (flag.cpu().numpy(), m.kernel_info())
        m.close()
        assert got[5]["vec"] == int(vec) and got[5]["threads"] == 256, got[5]
        tmask.assert_same(got, want, nrows, 1, 4096)


def case_id(case):
    return "-".join(str(v) for v in case)


COMPANION_RUNNERS = {"ddc": case_ddc, "corr": case_corr, "chan": case_chan, "demod": case_demod, "resamp": case_resamp,
                     "pulse": case_pulse, "iqfix": case_iqfix, "density": case_density, "detect": case_detect, "mask": case_mask}


@pytest.mark.parametrize("case", [c for c, _ in CASES], ids=case_id)
def test_recipe(ksa, torch_cuda, case):
    torch = torch_cuda
    family, args = case[0], case[1:]
    if family == "spectrum":
        case_spectrum(torch, ksa, *args)
    elif family == "pair":
        case_pair(torch, ksa, *args)
    elif family == "spectrum32":
        case_spectrum32(torch, ksa, *args)
    elif family == "spectrum64":
        case_spectrum64(torch, ksa, *args)
    elif family == "mr":
        case_mr(torch, ksa, *args)
    elif family == "dif":
        case_dif(torch, ksa, *args)
    elif family == "pfb_fold":
        case_pfb_fold(torch, ksa, *args)
    elif family == "pfb_ring":
        case_pfb_ring(torch, ksa, *args)
    elif family == "pfbpsd_fold":
        case_pfbpsd(torch, ksa, args[0], 3, ring=False)
    elif family == "pfbpsd_ring":
        case_pfbpsd(torch, ksa, args[0], args[1], ring=True)
    elif family in COMPANION_RUNNERS:
        load_pkg()
        COMPANION_RUNNERS[family](torch, importlib.import_module("prgs-sdr-kspecanal_amd." + family), *args)
    else:
        raise AssertionError("no runner for recipe %r" % (case,))


def test_every_recipe_family_has_a_runner():
    assert {c[0] for c, _ in CASES} == {"spectrum", "pair", "spectrum32", "spectrum64", "mr", "dif", "pfb_fold", "pfb_ring",
                                        "pfbpsd_fold", "pfbpsd_ring"} | set(COMPANION_RUNNERS)
