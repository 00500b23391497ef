"""GPU tests of the int8 / int16 sample formats (KSA_FMT_S8 = 2: b / 128, KSA_FMT_S16 = 3: b / 32768; interleaved I,Q, little-endian).

The yardstick is the pinned oracle fed the converted block, (a.astype(float32) / 128 or / 32768).view(complex64), under the
project's own bounds (assert_lin: 1e-5 normalised; assert_db).  On top of that, bit identity: the scale is a power of two and
commutes with every rounding, so on every path whose plan is the same for all formats the output must be np.array_equal to the
one of a complex64 engine fed the converted block -- every path except N = 64, where complex64 runs the 8 x 8 plan (path 5).
Covered: every kernel path and fold, frames / scan state, edge inputs, refusals, page-locked host memory as the IQ pointer of the
`_dev` calls (what SpectrumEngine.frames / curscan / frame / scan_pass do with int8 / int16 numpy arrays), the front end."""
import ctypes as C
import importlib
import re

import numpy as np
import pytest

import ksa_oracle as orc
import psd_helper
from conftest import load_pkg
from test_gpu_parity import assert_db, assert_lin, GAIN

pytestmark = pytest.mark.gpu
CURVES = ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg")
DIV = {"s8": 128.0, "s16": 32768.0}
DTYPE = {"s8": np.int8, "s16": np.int16}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def xres_for(n):
    """A waterfall width that divides fftSize (the reference's own fix-up gives 300 at fftSize 2400, K:937-949)."""
    return 512 if n % 512 == 0 or n < 512 else 300


def fmt_code(ksa, fmt):
    return {"s8": ksa.FMT_S8, "s16": ksa.FMT_S16}[fmt]


def convert(a, fmt):
    """The yardstick's input: the block as complex64, exactly (every int8 / int16 over a power of two is a float32)."""
    a = np.ascontiguousarray(a)
    return (a.astype(np.float32) / np.float32(DIV[fmt])).view(np.complex64)


def quantised(fmt, frames, full, seed, level=0.6):
    """[frames][2*full] int8 / int16: the oracle's synthetic tones + noise through the sources' quantiser."""
    x = orc.synth_iq(frames * full, seed) * level
    top = 127 if fmt == "s8" else 32767
    out = np.empty(2 * len(x), dtype=DTYPE[fmt])
    out[0::2] = np.clip(np.round(x.real * top), -top - 1, top)
    out[1::2] = np.clip(np.round(x.imag * top), -top - 1, top)
    return out.reshape(frames, 2 * full)


def random_ints(fmt, frames, full, seed):
    """Uniform over the whole range of the format, extremes included (fast: the large batches)."""
    info = np.iinfo(DTYPE[fmt])
    return np.random.default_rng(seed).integers(info.min, info.max + 1, (frames, 2 * full), dtype=DTYPE[fmt])


def curscan_dev(torch, eng, blocks, code, out_mode=0, stride=None):
    """ksa_curscan_dev on a device copy of `blocks` ([k][values]); c64 blocks are complex64 [k][full]."""
    k = blocks.shape[0]
    src = torch.view_as_real(torch.from_numpy(blocks)) if blocks.dtype == np.complex64 else torch.from_numpy(blocks)
    iq = src.to("cuda")
    out = torch.empty((k, eng.fft_size), dtype=torch.float32, device="cuda")
    eng.curscan_dev(iq, code, k, out, out_mode=out_mode, frame_stride=stride)
    eng.synchronize()
    return out.cpu().numpy()


def same_state(a, b, what, keys=CURVES + ("fftHM",), counters=("hm_index", "frames")):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), "%s: %s differs" % (what, k)
    for k in counters:
        assert a[k] == b[k], (what, k, a[k], b[k])


def oracle_lin(x, n, q, win, fold):
    if fold == "PSD":
        return psd_helper.psd(x, n, q, orc.window_table(win, n))
    return orc.curscan(x, n, q, orc.window_table(win, n), fold)


# ------------------------------------------------------------------------------------------------ every kernel path
# (fft_size, full_size, nonOverlap, window, frames, path reported for the engine; frames "big": more than twice the persistent grid)
PATHS = [
    (64, 512, 0.1, "hanning", 5, 5),            # complex64: the 8 x 8 plan; the narrow formats: the path-0 kernel
    (512, 4096, 0.5, "hanning", 5, 0),
    (1024, 8192, 0.5, "hamming", "big", 4),     # two frames per workgroup (the pair kernel)
    (4096, 32768, 0.5, "hanning", 1, 0),        # one block: the window split over workgroups
    (4096, 32768, 0.5, "hanning", "big", 0),    # persistent workgroups, sample reuse, the ping-pong loop
    (4096, 32768, 0.25, "kaiser", 3, 0),        # 75 % overlap: the rolled reuse loop
    (4096, 32768, 0.1, "hanning", 3, 0),        # fractional hops: the general path
    (8192, 65536, 0.5, "hanning", 2, 3),
    (16384, 131072, 0.5, "kaiser", 2, 3),
    (2400, 19200, 0.5, "hanning", 3, 6),
    (65536, 131072, 0.5, "hanning", 2, 2),      # radix-16 first stage
    (524288, 1048576, 0.5, "hamming", 1, 2),    # radix 32
    (1048576, 2097152, 0.5, "hanning", 1, 2),   # radix 64
]


@pytest.mark.parametrize("fmt", ["s8", "s16"])
@pytest.mark.parametrize("case", PATHS, ids=lambda c: "n%d_q%s_%s" % (c[0], c[2], c[4]))
def test_every_path_linear_vs_oracle_and_bit_identical_to_complex64(ksa, torch_cuda, case, fmt):
    torch = torch_cuda
    n, full, q, win, frames, path = case
    probe = ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window=win, xres=xres_for(n))
    info = probe.kernel_info()
    probe.close()
    assert info["path"] == path, info
    if frames == "big":
        frames = 2 * info["grid"] + 5
    blocks = random_ints(fmt, frames, full, n + frames) if frames > 8 else quantised(fmt, frames, full, n + frames)
    eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window=win, cumu_mode="AVG", max_frames=frames, xres=xres_for(n))
    got = curscan_dev(torch, eng, blocks, fmt_code(ksa, fmt))
    conv = np.stack([convert(b, fmt) for b in blocks])
    for f in sorted({0, frames // 2, frames - 1}):
        want = oracle_lin(conv[f], n, q, win, "AVG")
        assert_lin(got[f], want, what="N=%d %s frame %d" % (n, fmt, f))
    ref = curscan_dev(torch, eng, conv, ksa.FMT_C64)
    eng.close()
    if n == 64:      # complex64 takes another plan (8 x 8) there: the 1e-5 bound only
        for f in range(frames):
            assert_lin(got[f], ref[f], what="N=64 %s against the complex64 plan, frame %d" % (fmt, f))
    else:
        diff = np.max(np.abs(got.astype(np.float64) - ref)) / np.max(ref)
        print("N=%d q=%s %s: largest difference to the complex64 engine %.3g of the peak" % (n, q, fmt, diff))
        assert np.array_equal(got, ref), "N=%d %s: not bit-identical to complex64 (largest difference %.3g of the peak)" % (n, fmt, diff)


FOLD_CASES = [(512, 4096, 0.5, "hanning"), (4096, 32768, 0.5, "kaiser"), (16384, 131072, 0.25, "hanning"), (2400, 19200, 0.5, "hamming"),
              (65536, 131072, 0.5, "hanning")]


@pytest.mark.parametrize("fmt", ["s8", "s16"])
@pytest.mark.parametrize("fold", ["MAX", "MIN", "RAW", "PSD"])
@pytest.mark.parametrize("case", FOLD_CASES, ids=lambda c: "n%d" % c[0])
def test_folds_and_output_modes(ksa, torch_cuda, case, fold, fmt):
    """The MAX / MIN / RAW / PSD folds in LINEAR, OUT_DB and OUT_DB_CLIP units against the oracle, and against complex64 bit for bit."""
    torch = torch_cuda
    n, full, q, win = case
    frames = 3
    blocks = quantised(fmt, frames, full, 7 * n + len(fold))
    conv = np.stack([convert(b, fmt) for b in blocks])
    eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window=win, cumu_mode=fold, gain=GAIN, max_frames=frames, xres=xres_for(n))
    for mode in (ksa.OUT_LINEAR, ksa.OUT_DB, ksa.OUT_DB_CLIP):
        got = curscan_dev(torch, eng, blocks, fmt_code(ksa, fmt), out_mode=mode)
        ref = curscan_dev(torch, eng, conv, ksa.FMT_C64, out_mode=mode)
        assert np.array_equal(got, ref, equal_nan=True), "N=%d %s %s mode %d: not bit-identical to complex64" % (n, fold, fmt, mode)
        for f in (0, frames - 1):
            lin = oracle_lin(conv[f], n, q, win, fold)
            what = "N=%d %s %s mode %d frame %d" % (n, fold, fmt, mode, f)
            if mode == ksa.OUT_LINEAR:
                assert_lin(got[f], lin, what=what)
            elif mode == ksa.OUT_DB:
                assert_db(got[f], orc.log_no_gain(np.copy(lin), GAIN), what=what)
            else:
                assert_db(got[f], orc.log_no_gain(orc.clip2minamp(np.copy(lin), eng.min_amp), GAIN, inf_to=0), what=what)
    eng.close()


# ------------------------------------------------------------------------------------------------ state and scans
@pytest.mark.parametrize("fmt", ["s8", "s16"])
@pytest.mark.parametrize("case", [(512, 4096, 0.5, "hanning", 140), (4096, 32768, 0.5, "hanning", 9), (64, 512, 0.1, "ones", 40)],
                         ids=lambda c: "n%d" % c[0])
def test_frames_dev_state_equals_the_complex64_engine(ksa, torch_cuda, case, fmt):
    """Cur / Max / Min / Avg, the ring (more than 128 frames: it wraps), hm_index, frames_seen and the per-frame outputs, in two
    batches; against the oracle too."""
    torch = torch_cuda
    n, full, q, win, frames = case
    blocks = quantised(fmt, frames, full, 31 * n)
    conv = np.stack([convert(b, fmt) for b in blocks])
    mk = lambda: ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window=win, cumu_mode="AVG", gain=GAIN, xres=128, max_frames=frames)
    outs, states = [], []
    for src, code in ((blocks, fmt_code(ksa, fmt)), (conv, ksa.FMT_C64)):
        eng = mk()
        t = torch.view_as_real(torch.from_numpy(src)) if src.dtype == np.complex64 else torch.from_numpy(src)
        iq = t.to("cuda")
        db = torch.empty((frames, n), dtype=torch.float32, device="cuda")
        rows = torch.empty((frames, eng.hm_width), dtype=torch.float32, device="cuda")
        first = frames - 3
        eng.frames_dev(iq, code, first, cur_db=db, hm_rows=rows)
        eng.frames_dev(iq[first:], code, 3, cur_db=db[first:], hm_rows=rows[first:])
        eng.synchronize()
        outs.append((db.cpu().numpy(), rows.cpu().numpy()))
        states.append(eng.state())
        eng.close()
    st, _, _ = orc.zerospan_batch(conv, n, q, orc.window_table(win, n), "AVG", GAIN, 128)
    for k in ("Cur", "Max", "Min", "Avg"):
        assert_db(states[0]["Fft." + k], getattr(st, k.lower()), what="N=%d %s frames_dev %s" % (n, fmt, k))
    assert states[0]["hm_index"] == frames % 128 and states[0]["frames"] == frames
    if n == 64:
        for k in CURVES:
            assert_db(states[0][k], states[1][k], what="N=64 %s against the complex64 plan %s" % (fmt, k))
        return
    same_state(states[0], states[1], "N=%d %s frames_dev" % (n, fmt))
    for g, w, name in zip(outs[0], outs[1], ("cur_db", "hm_rows")):
        assert np.array_equal(g, w, equal_nan=True), "N=%d %s: per-frame %s differs" % (n, fmt, name)


@pytest.mark.parametrize("fmt", ["s8", "s16"])
def test_scan_pass_and_passes_with_a_failed_tune(ksa, torch_cuda, fmt):
    """ksa_scan_pass_dev / ksa_scan_passes_dev over a 3-band range, one band's tune failed in step_ok: the oracle's ScanState
    on the converted blocks, and the complex64 engine's state bit for bit."""
    torch = torch_cuda
    n, fs, start, end, passes = 512, 2.4e6, 99e6, 99e6 + 3 * 2.4e6, 3
    full = orc.full_size(n, fs)
    ref = orc.ScanState(n, start, end, fs, GAIN, (1 / 256) * 0.00001, 128)
    steps = len(ref.centers)
    blocks = quantised(fmt, passes * steps, full, 4711).reshape(passes, steps, 2 * full)
    conv = np.stack([convert(b, fmt) for b in blocks.reshape(passes * steps, -1)]).reshape(passes, steps, full)
    ok = np.ones((passes, steps), dtype=np.uint8)
    ok[1, 2] = 0
    win = orc.window_table("hanning", n)
    for p in range(passes):
        ref.run_pass([orc.curscan(conv[p, s], n, 0.1, win, "AVG") if ok[p, s] else None for s in range(steps)])
    mk = lambda: ksa.SpectrumEngine(n, full_size=full, non_overlap=0.1, window="hanning", gain=GAIN, xres=128, max_frames=passes * steps,
                                    scan_total_entries=ref.total, scan_non_overlap=0.5)
    states = {}
    for name, src, code in (("fixed", blocks, fmt_code(ksa, fmt)), ("c64", conv, ksa.FMT_C64)):
        flat = src.reshape(passes * steps, -1)
        t = torch.view_as_real(torch.from_numpy(flat)) if flat.dtype == np.complex64 else torch.from_numpy(flat)
        iq = t.to("cuda")
        eng = mk()                                     # pass by pass
        eng.scan_reset()
        for p in range(passes):
            eng.scan_pass_dev(iq[p * steps:], code, steps, step_ok=ok[p])
        eng.synchronize()
        states[name, "pass"] = eng.scan_state()
        eng.close()
        eng = mk()                                     # all passes in one call
        eng.scan_reset()
        eng.scan_passes_dev(iq, code, steps, passes, step_ok=ok.reshape(-1))
        eng.synchronize()
        states[name, "passes"] = eng.scan_state()
        eng.close()
    for how in ("pass", "passes"):
        got = states["fixed", how]
        for k in ("Cur", "Max", "Min", "Avg"):
            assert_db(got["Fft." + k], getattr(ref, k.lower()), what="%s scan %s %s" % (fmt, how, k))
        assert_db(got["fftHM"][:passes], ref.hm[:passes], what="%s scan %s waterfall" % (fmt, how))
        same_state(got, states["c64", how], "%s scan %s" % (fmt, how), counters=("hm_index", "passes"))
        assert got["passes"] == passes


@pytest.mark.parametrize("fmt", ["s8", "s16"])
def test_sharded_drivers_pass_the_format_through(ksa, torch_cuda, fmt):
    """distributed.ShardedZeroSpan.step and ShardedScan.run_pass with world size 1: no code of theirs knows the formats."""
    torch = torch_cuda
    D = importlib.import_module("prgs-sdr-kspecanal_amd.distributed")
    n, full, frames = 1024, 8192, 6
    blocks = quantised(fmt, frames, full, 99)
    conv = np.stack([convert(b, fmt) for b in blocks])
    mk = lambda: ksa.SpectrumEngine(n, full_size=full, non_overlap=0.5, window="hanning", gain=GAIN, xres=128, max_frames=frames)
    a, b = mk(), mk()
    D.ShardedZeroSpan(a).step(torch.from_numpy(blocks).to("cuda"), fmt_code(ksa, fmt), frames)
    b.frames_dev(torch.view_as_real(torch.from_numpy(conv)).to("cuda"), ksa.FMT_C64, frames)
    a.synchronize(), b.synchronize()
    same_state(a.state(), b.state(), "ShardedZeroSpan %s" % fmt)
    st, _, _ = orc.zerospan_batch(conv, n, 0.5, orc.window_table("hanning", n), "AVG", GAIN, 128)
    for k in ("Cur", "Max", "Min", "Avg"):
        assert_db(a.state()["Fft." + k], getattr(st, k.lower()), what="ShardedZeroSpan %s %s" % (fmt, k))
    a.close(), b.close()
    # band-sharded scan, one rank
    fs, start, end = 2.4e6, 99e6, 99e6 + 3 * 2.4e6
    n, full = 512, orc.full_size(512, fs)
    ref = orc.ScanState(n, start, end, fs, GAIN, (1 / 256) * 0.00001, 128)
    steps = len(ref.centers)
    blocks = quantised(fmt, steps, full, 123)
    conv = np.stack([convert(x, fmt) for x in blocks])
    ref.run_pass([orc.curscan(c, n, 0.1, orc.window_table("hanning", n), "AVG") for c in conv])
    eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=0.1, window="hanning", gain=GAIN, xres=128, max_frames=steps,
                             scan_total_entries=ref.total, scan_non_overlap=0.5)
    eng.scan_reset()
    D.ShardedScan(eng).run_pass(torch.from_numpy(blocks).to("cuda"), fmt_code(ksa, fmt), steps)
    eng.synchronize()
    got = eng.scan_state()
    for k in ("Cur", "Max", "Min", "Avg"):
        assert_db(got["Fft." + k], getattr(ref, k.lower()), what="ShardedScan %s %s" % (fmt, k))
    eng.close()


# ------------------------------------------------------------------------------------------------ edge inputs
@pytest.mark.parametrize("fmt", ["s8", "s16"])
@pytest.mark.parametrize("n,full,q", [(512, 4096, 0.5), (4096, 32768, 0.5), (2400, 19200, 0.5), (65536, 131072, 0.5)])
def test_extreme_values_zero_blocks_and_an_odd_stride(ksa, torch_cuda, fmt, n, full, q):
    torch = torch_cuda
    info = np.iinfo(DTYPE[fmt])
    rng = np.random.default_rng(n)
    code = fmt_code(ksa, fmt)
    # a block of nothing but the two extremes (-32768 / 32767, -128 / 127), a block at the negative rail, a zero block
    blocks = np.zeros((3, 2 * full), dtype=DTYPE[fmt])
    blocks[0] = np.where(rng.integers(0, 2, 2 * full) == 1, info.max, info.min)
    blocks[1] = info.min
    conv = np.stack([convert(b, fmt) for b in blocks])
    assert conv[1][0] == complex(-1, -1) and np.max(conv[0].real) == info.max / DIV[fmt]
    eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window="hanning", cumu_mode="AVG", gain=GAIN, min_amp=0.0, max_frames=3, xres=xres_for(n))
    lin = curscan_dev(torch, eng, blocks, code)
    for f in (0, 1):
        assert_lin(lin[f], orc.curscan(conv[f], n, q, orc.window_table("hanning", n), "AVG"), what="N=%d %s extremes block %d" % (n, fmt, f))
    assert np.array_equal(lin, curscan_dev(torch, eng, conv, ksa.FMT_C64))
    assert np.all(lin[2] == 0.0)
    db = curscan_dev(torch, eng, blocks, code, out_mode=ksa.OUT_DB)
    assert np.all(np.isneginf(db[2])), "an all-zero block is -inf dB"
    clip = curscan_dev(torch, eng, blocks, code, out_mode=ksa.OUT_DB_CLIP)
    assert np.all(clip[2] == 0.0), "an all-zero block is 0 under OUT_DB_CLIP with min_amp 0"
    eng.close()
    # an odd frame_stride (in samples): frames overlap in memory and start off the wider alignments
    stride = full // 2 + 7
    flat = quantised(fmt, 1, 2 * stride + full, n + 1)[0]
    eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window="hanning", cumu_mode="MAX", max_frames=3, xres=xres_for(n))
    iq = torch.from_numpy(flat).to("cuda")
    out = torch.empty((3, n), dtype=torch.float32, device="cuda")
    eng.curscan_dev(iq, code, 3, out, frame_stride=stride)
    eng.synchronize()
    got = out.cpu().numpy()
    for f in range(3):
        x = convert(flat[2 * f * stride:2 * (f * stride + full)], fmt)
        assert_lin(got[f], orc.curscan(x, n, q, orc.window_table("hanning", n), "MAX"), what="N=%d %s odd stride frame %d" % (n, fmt, f))
    cflat = convert(flat, fmt)
    ciq = torch.view_as_real(torch.from_numpy(cflat)).to("cuda")
    eng.curscan_dev(ciq, ksa.FMT_C64, 3, out, frame_stride=stride)
    eng.synchronize()
    assert np.array_equal(got, out.cpu().numpy()), "N=%d %s odd stride: not bit-identical to complex64" % (n, fmt)
    eng.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_state_alone_and_write_their_own_text(ksa, torch_cuda):
    torch = torch_cuda
    n, full = 512, 4096
    eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=0.5, window="hanning", gain=GAIN, xres=128, max_frames=4,
                             scan_total_entries=3 * n, scan_non_overlap=0.5)
    blocks = quantised("s16", 4, full, 5)
    iq = torch.zeros(2 * 4 * full + 8, dtype=torch.int16, device="cuda")
    iq[:2 * 4 * full] = torch.from_numpy(blocks.reshape(-1)).to("cuda")
    out = torch.empty((4, n), dtype=torch.float32, device="cuda")
    eng.frames_dev(iq, ksa.FMT_S16, 4)
    eng.synchronize()
    before = eng.state()
    lib, h = ksa.lib, eng._h
    base = iq.data_ptr()
    assert base % 4 == 0
    calls = {
        "curscan": lambda p, f: lib.ksa_curscan_dev(h, C.c_void_p(p), f, full, 2, 0, C.c_void_p(out.data_ptr())),
        "frames": lambda p, f: lib.ksa_frames_dev(h, C.c_void_p(p), f, full, 2, 0, 2, None, None, 1),
        "scan_pass": lambda p, f: lib.ksa_scan_pass_dev(h, C.c_void_p(p), f, full, 3, None),
        "scan_passes": lambda p, f: lib.ksa_scan_passes_dev(h, C.c_void_p(p), f, full, 3, 1, None),
        "scan_spectra": lambda p, f: lib.ksa_scan_spectra_dev(h, C.c_void_p(p), f, full, 2, None, C.c_void_p(out.data_ptr())),
    }
    scan_before = eng.scan_state()
    for name, call in calls.items():
        for ptr, fmt, word in ((base + 2, ksa.FMT_S16, b"not sample aligned"), (base + 1, ksa.FMT_S8, b"not sample aligned"),
                               (base, 4, b"unknown sample format"), (base, -1, b"unknown sample format")):
            lib.ksa_merge_gathered_dev(h, C.c_void_p(base), 0, 1, 0)      # leaves "world 0 < 1" behind: each refusal writes its own text
            rc = call(ptr, fmt)
            err = lib.ksa_last_error()
            assert rc != 0 and word in err, (name, fmt, err)
            same_state(eng.state(), before, "after refused %s fmt %d" % (name, fmt))
            same_state(eng.scan_state(), scan_before, "scan after refused %s fmt %d" % (name, fmt), counters=("hm_index", "passes"))
    # 2-byte alignment is enough for int8, and the right alignments are accepted by every entry point
    for name, call in calls.items():
        assert call(base + 2, ksa.FMT_S8) == 0, (name, lib.ksa_last_error())
        assert call(base + 4, ksa.FMT_S16) == 0, (name, lib.ksa_last_error())
    eng.synchronize()
    eng.close()


# ------------------------------------------------------------------------------------------------ page-locked host memory
@pytest.mark.parametrize("fmt", ["s8", "s16"])
@pytest.mark.parametrize("case", [(512, 4096, 0.5, 40), (4096, 32768, 0.5, 9), (16384, 131072, 0.5, 3), (65536, 131072, 0.5, 3)],
                         ids=lambda c: "n%d" % c[0])
def test_pinned_host_memory_as_the_iq_pointer(ksa, torch_cuda, case, fmt):
    """The same bytes in a PinnedBuffer and in device memory: array_equal state and outputs from ksa_frames_dev / ksa_curscan_dev."""
    torch = torch_cuda
    n, full, q, frames = case
    blocks = quantised(fmt, frames, full, 17 * n)
    code = fmt_code(ksa, fmt)
    mk = lambda: ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window="hanning", gain=GAIN, xres=128, max_frames=frames)
    dev, pin = mk(), mk()
    iq = torch.from_numpy(blocks).to("cuda")
    pb = ksa.PinnedBuffer(blocks.shape, blocks.dtype)
    pb.array[...] = blocks
    outs = []
    for eng, src in ((dev, iq), (pin, pb.array)):
        db = torch.empty((frames, n), dtype=torch.float32, device="cuda")
        lin = torch.empty((frames, n), dtype=torch.float32, device="cuda")
        eng.frames_dev(src, code, frames, cur_db=db)
        eng.curscan_dev(src, code, frames, lin)
        eng.synchronize()
        outs.append((db.cpu().numpy(), lin.cpu().numpy()))
    same_state(pin.state(), dev.state(), "N=%d %s pinned IQ pointer" % (n, fmt))
    assert np.array_equal(outs[0][0], outs[1][0], equal_nan=True) and np.array_equal(outs[0][1], outs[1][1])
    assert np.array_equal(pb.array, blocks), "the caller's buffer changed"
    dev.close(), pin.close(), pb.close()


@pytest.mark.parametrize("fmt", ["s8", "s16"])
def test_engine_methods_take_int8_and_int16_numpy_arrays(ksa, torch_cuda, fmt):
    """SpectrumEngine.frames / frame / curscan / scan_pass on plain numpy arrays (staged in an engine-owned PinnedBuffer) and on
    PinnedBuffer.array (handed over as it is): the state of the `_dev` form on a device copy; results valid on return."""
    torch = torch_cuda
    n, full, q, frames = 1024, 8192, 0.5, 21
    blocks = quantised(fmt, frames, full, 1234)
    conv = np.stack([convert(b, fmt) for b in blocks])
    code = fmt_code(ksa, fmt)
    mk = lambda: ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window="hanning", gain=GAIN, xres=128, max_frames=frames)
    ref = mk()
    iq = torch.from_numpy(blocks).to("cuda")
    db = torch.empty((frames, n), dtype=torch.float32, device="cuda")
    rows = torch.empty((frames, ref.hm_width), dtype=torch.float32, device="cuda")
    ref.frames_dev(iq, code, frames, cur_db=db, hm_rows=rows)
    ref.synchronize()
    want = ref.state()
    pb = ksa.PinnedBuffer(blocks.shape, blocks.dtype)
    pb.array[...] = blocks
    for kind, arr in (("pageable", blocks), ("pinned", pb.array), ("strided", np.repeat(blocks, 2, axis=0)[::2])):
        eng = mk()
        got_db, got_rows = eng.frames(arr, cur_db=True, hm_rows=True)
        same_state(eng.state(), want, "%s frames(%s)" % (fmt, kind))
        assert np.array_equal(got_db, db.cpu().numpy(), equal_nan=True) and np.array_equal(got_rows, rows.cpu().numpy(), equal_nan=True)
        assert eng.frames(arr[:2]) == (None, None)
        eng.close()
    assert np.array_equal(pb.array, blocks)
    # frame by frame == the batch's curves up to the batch's own plan (another window split): the oracle decides
    eng = mk()
    for b in blocks[:5]:
        eng.frame(b)
    st, _, _ = orc.zerospan_batch(conv[:5], n, q, orc.window_table("hanning", n), "AVG", GAIN, 128)
    for k in ("Cur", "Max", "Min", "Avg"):
        assert_db(eng.state()["Fft." + k], getattr(st, k.lower()), what="%s frame() %s" % (fmt, k))
    assert eng.state()["frames"] == 5
    # curscan: float64 linear magnitudes of one block
    y = eng.curscan(blocks[3])
    assert y.dtype == np.float64 and y.shape == (n,)
    assert_lin(y, orc.curscan(conv[3], n, q, orc.window_table("hanning", n), "AVG"), what="%s curscan()" % fmt)
    assert np.array_equal(y, eng.curscan(conv[3])), "curscan(%s) differs from curscan(complex64)" % fmt
    with pytest.raises(ksa.KsaError):
        eng.curscan(blocks[3][:-2])
    with pytest.raises(ksa.KsaError):
        eng.frames(blocks.reshape(-1))
    eng.close(), ref.close(), pb.close()
    # scan_pass with a failed tune
    fs, start, end = 2.4e6, 99e6, 99e6 + 3 * 2.4e6
    n, full = 512, orc.full_size(512, fs)
    sref = orc.ScanState(n, start, end, fs, GAIN, (1 / 256) * 0.00001, 128)
    steps = len(sref.centers)
    sblocks = quantised(fmt, 2 * steps, full, 77).reshape(2, steps, 2 * full)
    ok = np.ones((2, steps), dtype=np.uint8)
    ok[0, 1] = 0
    win = orc.window_table("hanning", n)
    eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=0.1, window="hanning", gain=GAIN, xres=128, max_frames=steps,
                             scan_total_entries=sref.total, scan_non_overlap=0.5)
    eng.scan_reset()
    for p in range(2):
        sref.run_pass([orc.curscan(convert(sblocks[p, s], fmt), n, 0.1, win, "AVG") if ok[p, s] else None for s in range(steps)])
        eng.scan_pass(sblocks[p], step_ok=ok[p])
    got = eng.scan_state()
    for k in ("Cur", "Max", "Min", "Avg"):
        assert_db(got["Fft." + k], getattr(sref, k.lower()), what="%s scan_pass() %s" % (fmt, k))
    assert got["passes"] == 2
    eng.close()


# ------------------------------------------------------------------------------------------------ the front end
def _K():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")


def _capture(tmp_path, fmt, layout, seed, name):
    """A capture file of format `fmt`: per block `settle` samples that sdr_setup discards (K:301), then `full` samples.
    layout = [(settle, full), ...].  Returns (path, the blocks as converted complex64)."""
    total = sum(s + f for s, f in layout)
    raw = quantised(fmt, 1, total, seed, level=0.7)[0]
    path = tmp_path / name
    raw.tofile(path)
    blocks, pos = [], 0
    for settle, full in layout:
        pos += settle
        blocks.append(convert(raw[2 * pos:2 * (pos + full)], fmt))
        pos += full
    return str(path), blocks


def _run(K, capsys, argv):
    K.sdr_curscan = K._gpu_curscan
    capsys.readouterr()
    d = K.main(argv)
    out = capsys.readouterr().out
    return d, len(re.findall(r"^ZeroSpan:\d+:", out, flags=re.M))


def test_front_end_zero_span_from_an_int16_capture(ksa, torch_cuda, tmp_path, capsys):
    """`zeroSpan iqFormat s16 source file:...` at frameBatch 1 and 64 against the oracle on the converted capture; a capture
    that ends mid-batch stops after the same frames as frameBatch 1; curScanCumuMode psd and bUsePSD keep working."""
    K = _K()
    n, frames = 4096, 150
    full = orc.full_size(n, 2.4e6)
    path, blocks = _capture(tmp_path, "s16", [(16 * 1024, full)] + [(0, full)] * (frames - 1), 2024, "cap_s16.bin")
    st, _, _ = orc.zerospan_batch(np.array(blocks), n, 0.5, orc.window_table("hanning", n), "AVG", 19.1, 512)
    common = ["zeroSpan", "fftSize", str(n), "window", "hanning", "curScanNonOverlap", "0.5", "bPltLevels", "false",
              "bPltHeatMap", "false", "source", "file:%s" % path, "iqFormat", "s16"]
    for batch, lines in (("1", frames), ("64", 3)):
        d, seen = _run(K, capsys, common + ["prgLoopCnt", str(frames), "frameBatch", batch])
        for k in ("Cur", "Max", "Min", "Avg"):
            assert_db(d["Fft." + k], getattr(st, k.lower()), what="s16 frameBatch %s %s" % (batch, k))
        assert d["fftHMIndex"] == frames % 128 and seen == lines
    # the capture ends mid-batch: the same frames as frameBatch 1, then the run stops
    d1, _ = _run(K, capsys, common + ["prgLoopCnt", "400", "frameBatch", "1"])
    d64, lines = _run(K, capsys, common + ["prgLoopCnt", "400", "frameBatch", "64"])
    assert d1["cmd.stop"] is True and d64["cmd.stop"] is True and lines == 3
    for k in CURVES:
        assert_db(d64[k], d1[k], what="short s16 capture " + k)
        assert_db(d64[k], getattr(st, k[4:].lower()), what="short s16 capture vs oracle " + k)
    # curScanCumuMode psd, and the bUsePSD diagnostic, on int16 blocks
    few = 4
    win = orc.window_table("hanning", n)
    pst = orc.ZeroSpanState(n, 512, 19.1)
    for b in blocks[:few]:
        pst.push(psd_helper.psd(b, n, 0.5, win))
    d, _ = _run(K, capsys, common + ["prgLoopCnt", str(few), "curScanCumuMode", "psd"])
    for k in ("Cur", "Max", "Min", "Avg"):
        assert_db(d["Fft." + k], getattr(pst, k.lower()), what="s16 psd fold %s" % k)
    try:
        import matplotlib  # noqa: F401  (the bUsePSD diagnostic is matplotlib's Welch PSD; without the package there is nothing to run)
    except ImportError:
        return
    d, _ = _run(K, capsys, common + ["prgLoopCnt", "2", "bUsePSD", "true"])
    kg, kp, lg, lp = d["psd.check"]
    assert kg == kp and abs(lg - lp) < 0.2          # the bound of test_gpu_round2.py's diagnostic test


def test_front_end_scan_from_an_int8_capture(ksa, torch_cuda, tmp_path, capsys):
    """A 3-band scan with iqFormat s8 over a file capture (every step: 16Ki settle samples, then the block)."""
    K = _K()
    n, fs, passes = 512, 2.4e6, 2
    full = orc.full_size(n, fs)
    ref = orc.ScanState(n, 99e6, 99e6 + 3 * fs, fs, 19.1, (1 / 256) * 0.00001, 128)
    steps = len(ref.centers)
    path, blocks = _capture(tmp_path, "s8", [(16 * 1024, full)] * (passes * steps), 31337, "cap_s8.bin")
    win = orc.window_table("hanning", n)
    for p in range(passes):
        ref.run_pass([orc.curscan(b, n, 0.1, win, "AVG") for b in blocks[p * steps:(p + 1) * steps]])
    d, _ = _run(K, capsys, ["scan", "startFreq", "99e6", "endFreq", "106e6", "fftSize", str(n), "window", "hanning", "prgLoopCnt", str(passes),
                            "xRes", "128", "bPltLevels", "false", "bPltHeatMap", "false", "source", "file:%s" % path, "iqFormat", "s8"])
    for k in ("Cur", "Max", "Min", "Avg"):
        assert_db(d["Fft." + k], getattr(ref, k.lower()), what="s8 scan " + k)
    assert_db(d["fftHM"][:passes], ref.hm[:passes], what="s8 scan waterfall")
    # the synthetic source's quantisers feed the same route
    d, _ = _run(K, capsys, ["zeroSpan", "fftSize", "512", "window", "kaiser", "prgLoopCnt", "3", "iqFormat", "s8", "frameBatch", "2",
                            "bPltLevels", "false", "bPltHeatMap", "false", "source", "synth"])
    assert d["fftHMIndex"] == 3 and np.all(np.isfinite(d["Fft.Avg"]))
