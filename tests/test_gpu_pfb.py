"""GPU tests of the polyphase filter bank front end (KSA_CUMU_PFB, SpectrumEngine(pfb_taps=...), pfbTaps): every transform path
behind the fold, the ring kernel against the generic one bit for bit, the exact integer formats, special blocks, zeroSpan state
through the device and host batch entries, a scan pass and the front end -- against the float64 model of pfb_helper.py.

Tolerances are the project's own: assert_lin (1e-5 of the strongest bin) and assert_db exactly as they stand."""
import importlib
import os
import re

import numpy as np
import pytest

import ksa_oracle as orc
import pfb_helper as pfb
from conftest import ROOT, load_pkg
from test_gpu_parity import assert_lin, assert_db, GAIN

pytestmark = pytest.mark.gpu
CURVES = ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg")
SLICE = int(re.search(r"constexpr int PFB_SLICE_FRAMES = (\d+);",
                      open(os.path.join(ROOT, "prgs-sdr-kspecanal_amd", "csrc", "ksa_pfb.hpp")).read()).group(1))
CHUNK_BYTES = int(re.search(r"#define KSA_PFB_CHUNK_BYTES \((\d+)ll << 20\)",
                            open(os.path.join(ROOT, "prgs-sdr-kspecanal_amd", "csrc", "ksa_api.hip")).read()).group(1)) << 20


def chunk_frames(n):
    """Frames of one fold + transform chunk at fftSize n for an engine whose max_frames is larger (ksa_create)."""
    return max(4, CHUNK_BYTES // (8 * n) // 4 * 4)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


_BASE = {}


def _stream(total, seed=4242):
    """`total` samples of the oracle's synthetic IQ.  Long streams repeat one 2^21-sample draw with a shift and a level per
    repeat (the generator costs 0.3 us per sample; the tests only need blocks that differ)."""
    unit = 1 << 21
    if total <= unit:
        return (orc.synth_iq(total, seed + total) * 0.7).astype(np.complex64)
    if seed not in _BASE:
        _BASE[seed] = (orc.synth_iq(unit, seed) * 0.7).astype(np.complex64)
    base = _BASE[seed]
    parts = [np.roll(base, 4099 * k) * np.float32(1.0 - 0.07 * (k % 5)) for k in range(-(-total // unit))]
    return np.concatenate(parts)[:total]


def _xres(n):
    return n if n & (n - 1) else min(n, 512)


def _dev(torch, x):
    x = np.ascontiguousarray(x)
    if x.dtype == np.complex64:
        return torch.view_as_real(torch.from_numpy(x)).to("cuda")
    return torch.from_numpy(x).to("cuda")


# (N, P, window of the prototype, frames, path of kernel_info, what the case is there for)
# frames: an int, or "pair" / "fill" / "chunk": as many as the pair kernel (path 4) or a filled launch needs, or three more than
# one fold + transform chunk holds (the second chunk then starts at a frame that is no multiple of anything else in the plan)
PATHS = [
    (16, 2, "hamming", 5, 0, "M = 1; P = 2 is the generic kernel"),
    (32, 3, "hanning", 5, 0, "generic kernel at stride N (P = 3)"),
    (64, 4, "hamming", 7, 5, "rectangular 8 x 8 plan for both formats"),
    (128, 5, "kaiser", 4, 0, "generic kernel (P = 5)"),
    (512, 4, "hanning", 2 * SLICE + 3, 0, "three ring slices (complex64; uint8 at P = 4 is the generic kernel)"),
    (1024, 8, "hamming", "pair", 4, "pair kernel behind the fold"),
    (2048, 2, "ones", 3, 0, ""),
    (4096, 4, "hanning", 1, 0, "one frame"),
    (4096, 4, "hamming", "fill", 0, "filled launch"),
    (8192, 2, "hanning", 3, 3, "32 points per thread"),
    (16384, 4, "hamming", 2, 3, "32 points per thread"),
    (32768, 2, "hanning", 2, 2, "radix-16 first stage"),
    (65536, 2, "hamming", 2, 2, "radix-16 first stage, 4096-point second stage"),
    (524288, 2, "hanning", 2, 2, "radix-32 first stage"),
    (1048576, 2, "hamming", "chunk", 2, "radix-64 first stage; two fold + transform chunks (32 + 3 frames at 256 MiB)"),
    (20, 3, "hanning", 4, 6, "mixed radix 4 * 5"),
    (1000, 4, "hamming", 3, 6, "mixed radix"),
    (2400, 16, "hanning", 3, 6, "mixed radix, 16 taps"),
    (16200, 2, "kaiser", 2, 6, "mixed radix, the largest plan"),
]


@pytest.mark.parametrize("case", PATHS, ids=["%d-%d-%s" % (c[0], c[1], c[3]) for c in PATHS])
def test_curscan_dev_linear_on_every_path(ksa, torch_cuda, case):
    """Frames at stride N over one sample stream (the critically sampled PFB): complex64 and uint8 input, linear output."""
    torch = torch_cuda
    n, p, window, frames, path, _ = case
    probe = ksa.SpectrumEngine(n, pfb_taps=p, window=window, xres=_xres(n))
    info = probe.kernel_info()
    probe.close()
    assert info["path"] == path, info
    if frames == "pair":
        frames = 2 * info["grid"] + 1
    elif frames == "fill":
        frames = info["grid"] // 2 + 3
    edge = set()
    if frames == "chunk":
        frames = chunk_frames(n) + 3
        edge = {chunk_frames(n) - 1, chunk_frames(n)}
    x = _stream((frames - 1 + p) * n)
    raw = orc.quantize_u8(x)
    eng = ksa.SpectrumEngine(n, pfb_taps=p, window=window, xres=_xres(n), max_frames=frames)
    taps = pfb.prototype(n, p, window)
    assert np.array_equal(eng.win, taps) and eng.mag_scale == pfb.scale(taps) and eng.full_size == p * n
    assert np.array_equal(eng.starts, np.arange(p) * n)
    out = torch.empty((frames, n), dtype=torch.float32, device="cuda")
    check = sorted(set(np.linspace(0, frames - 1, min(frames, 4 if edge else 6)).astype(int)) | edge)
    for fmt, src in ((ksa.FMT_C64, x), (ksa.FMT_U8, raw)):
        out.fill_(-1.0)
        eng.curscan_dev(_dev(torch, src), fmt, frames, out, frame_stride=n)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.all(got >= 0), "a frame was not written"
        for f in check:
            block = x[f * n:(f + p) * n] if fmt == ksa.FMT_C64 else orc.unpack_u8(raw[2 * f * n:2 * (f + p) * n])
            want = pfb.spectrum(block, n, taps)
            assert_lin(got[f], want, what="N=%d P=%d %s fmt %d frame %d/%d" % (n, p, window, fmt, f, frames))
    eng.close()


def _quantized(ksa, x, fmt):
    """The samples of the complex stream `x` in format fmt, as the array handed to the device."""
    if fmt == ksa.FMT_C64:
        return x
    if fmt == ksa.FMT_U8:
        return orc.quantize_u8(x)
    bits, dtype = (7, np.int8) if fmt == ksa.FMT_S8 else (15, np.int16)
    v = np.empty(2 * len(x), dtype=np.float64)
    v[0::2], v[1::2] = x.real, x.imag
    return np.clip(np.round(v * (1 << bits)), -(1 << bits), (1 << bits) - 1).astype(dtype)


@pytest.mark.parametrize("p", [2, 4, 8, 16])
def test_ring_kernel_equals_the_generic_kernel_bit_for_bit(ksa, torch_cuda, p):
    """Stride N over the stream against the same frames materialised as blocks [frames][P*N] at stride P*N (always the generic
    kernel): array_equal, every sample format, frame counts 1, P-1, P and two whole ring slices plus three frames.  Stride N
    takes the ring kernel where (P - 1) * bytes per sample >= 12 (complex64 from P = 4, int16 from P = 4, the 2-byte formats
    from P = 8) and the generic kernel below that."""
    torch = torch_cuda
    n = 256
    counts = sorted({1, p - 1, p, 2 * SLICE + 3})
    most = counts[-1]
    x = _stream((most - 1 + p) * n, seed=77 + p)
    eng = ksa.SpectrumEngine(n, pfb_taps=p, window="hamming", xres=64, max_frames=most)
    for fmt in (ksa.FMT_C64, ksa.FMT_U8, ksa.FMT_S8, ksa.FMT_S16):
        q = _quantized(ksa, x, fmt)
        per = 1 if fmt == ksa.FMT_C64 else 2               # array elements per sample
        blocks = np.stack([q[f * n * per:(f + p) * n * per] for f in range(most)])
        d_stream, d_blocks = _dev(torch, q), _dev(torch, blocks.reshape(-1))
        for frames in counts:
            a = torch.full((frames, n), -1.0, dtype=torch.float32, device="cuda")
            b = torch.full((frames, n), -2.0, dtype=torch.float32, device="cuda")
            eng.curscan_dev(d_stream, fmt, frames, a, frame_stride=n)
            eng.curscan_dev(d_blocks, fmt, frames, b, frame_stride=p * n)
            torch.cuda.synchronize()
            a, b = a.cpu().numpy(), b.cpu().numpy()
            assert np.all(a >= 0) and np.array_equal(a, b), "P=%d fmt %d frames %d" % (p, fmt, frames)
    eng.close()


@pytest.mark.parametrize("p", [3, 4])
def test_integer_formats_equal_complex64_of_the_same_values(ksa, torch_cuda, p):
    """int8 / int16 samples are b / 128 and b / 32768, exact in float32: the complex64 run of those values gives the same bits
    (P = 4: the ring kernel for int16 and complex64, the generic kernel for int8; P = 3: the generic kernel)."""
    torch = torch_cuda
    n, frames = 512, 9
    x = _stream((frames - 1 + p) * n, seed=5)
    eng = ksa.SpectrumEngine(n, pfb_taps=p, window="hanning", xres=64, max_frames=frames)
    for fmt, div in ((ksa.FMT_S8, 128.0), (ksa.FMT_S16, 32768.0)):
        q = _quantized(ksa, x, fmt)
        same = (q.astype(np.float32) / np.float32(div)).view(np.complex64)
        a = torch.empty((frames, n), dtype=torch.float32, device="cuda")
        b = torch.empty((frames, n), dtype=torch.float32, device="cuda")
        eng.curscan_dev(_dev(torch, q), fmt, frames, a, frame_stride=n)
        eng.curscan_dev(_dev(torch, same), ksa.FMT_C64, frames, b, frame_stride=n)
        torch.cuda.synchronize()
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()), "fmt %d" % fmt
        assert_lin(a.cpu().numpy()[frames - 1], pfb.spectrum(same[(frames - 1) * n:].astype(np.complex128), n, eng.win), what="fmt %d" % fmt)
    eng.close()


@pytest.mark.parametrize("n", [64, 2400, 4096, 32768])
def test_zero_block_and_nan_sample(ksa, torch_cuda, n):
    """Three blocks [3][P*N]: a signal, all zero, one NaN in the last segment.  The NaN reaches every bin of its frame and no
    other frame; the zero block reads -inf under OUT_DB and 0 under OUT_DB_CLIP with min_amp 0."""
    torch = torch_cuda
    p = 4
    x = _stream(3 * p * n, seed=9).reshape(3, p * n).copy()
    x[1] = 0
    x[2, (p - 1) * n + n // 3] = np.nan
    eng = ksa.SpectrumEngine(n, pfb_taps=p, window="hanning", gain=GAIN, min_amp=0.0, xres=_xres(n), max_frames=3)
    want = pfb.spectrum(x[0], n, eng.win)
    dev = _dev(torch, x.reshape(-1))
    out = torch.empty((3, n), dtype=torch.float32, device="cuda")
    res = {}
    for mode in (ksa.OUT_LINEAR, ksa.OUT_DB, ksa.OUT_DB_CLIP):
        eng.curscan_dev(dev, ksa.FMT_C64, 3, out, out_mode=mode)
        torch.cuda.synchronize()
        res[mode] = out.cpu().numpy()
    eng.close()
    assert_lin(res[ksa.OUT_LINEAR][0], want, what="N=%d linear" % n)
    assert_db(res[ksa.OUT_DB][0], orc.log_no_gain(np.copy(want), GAIN), what="N=%d OUT_DB" % n)
    assert_db(res[ksa.OUT_DB_CLIP][0], orc.log_no_gain(orc.clip2minamp(np.copy(want), 0.0), GAIN, inf_to=0), what="N=%d OUT_DB_CLIP" % n)
    assert np.all(res[ksa.OUT_LINEAR][1] == 0) and np.all(np.isneginf(res[ksa.OUT_DB][1])) and np.all(res[ksa.OUT_DB_CLIP][1] == 0)
    for mode in res:
        assert np.all(np.isnan(res[mode][2])) and not np.any(np.isnan(res[mode][:2])), mode


def _check_state(got, st, what, frames):
    for k in CURVES:
        assert_db(got[k], getattr(st, k[4:].lower()), what="%s %s" % (what, k))
    assert_db(got["fftHM"], st.hm, what=what + " ring")
    assert got["hm_index"] == frames % 128 and got["frames"] == frames


@pytest.mark.parametrize("n,p,frames", [(512, 4, 200)])
def test_zerospan_state_at_stride_n(ksa, torch_cuda, n, p, frames):
    """ksa_frames_dev over a stream at stride N against ZeroSpanState fed with the model's per-frame spectra: 200 frames wrap the
    128-row ring.  Then the same run fed in two calls to a second engine with a larger max_frames: per-frame spectra and
    waterfall rows, Cur, Max, Min and the ring the same bits.  Avg is held to the oracle only: the engine's batched accumulate
    (the closed form of the (a + x) / 2 recursion per call, in every fold mode) rounds Avg differently when a run is cut into
    other calls.  That fold + transform CHUNKS inside one call change nothing, Avg included, is
    test_chunked_batch_equals_one_launch_bit_for_bit."""
    torch = torch_cuda
    xres = 64
    x = _stream((frames - 1 + p) * n, seed=31)
    taps = pfb.prototype(n, p, "hamming")
    st = orc.ZeroSpanState(n, xres, GAIN)
    db_ref = np.array([st.push(pfb.spectrum(x[f * n:(f + p) * n], n, taps)) for f in range(frames)])
    dev = _dev(torch, x)
    one = ksa.SpectrumEngine(n, pfb_taps=p, window="hamming", gain=GAIN, xres=xres, max_frames=frames)
    db = torch.empty((frames, n), dtype=torch.float32, device="cuda")
    rows = torch.empty((frames, xres), dtype=torch.float32, device="cuda")
    one.frames_dev(dev, ksa.FMT_C64, frames, cur_db=db, hm_rows=rows, frame_stride=n)
    one.synchronize()
    got = one.state()
    one.close()
    _check_state(got, st, "one call", frames)
    assert_db(db.cpu().numpy(), db_ref, what="per-frame dB")
    assert_db(rows.cpu().numpy(), np.array([orc.plotcompress(r, xres, "MAX") for r in db_ref]), what="per-frame rows")
    two = ksa.SpectrumEngine(n, pfb_taps=p, window="hamming", gain=GAIN, xres=xres, max_frames=2 * frames)
    db2 = torch.empty((frames, n), dtype=torch.float32, device="cuda")
    rows2 = torch.empty((frames, xres), dtype=torch.float32, device="cuda")
    cut = frames // 2 + 1
    two.frames_dev(dev, ksa.FMT_C64, cut, cur_db=db2, hm_rows=rows2, frame_stride=n)
    two.frames_dev(dev[cut * n:], ksa.FMT_C64, frames - cut, cur_db=db2[cut:], hm_rows=rows2[cut:], frame_stride=n)
    two.synchronize()
    got2 = two.state()
    two.close()
    assert torch.equal(db, db2) and torch.equal(rows, rows2)
    for k in ("Fft.Cur", "Fft.Max", "Fft.Min"):
        assert np.array_equal(got[k], got2[k]), k
    assert np.array_equal(got["fftHM"], got2["fftHM"]) and got2["hm_index"] == frames % 128 and got2["frames"] == frames
    assert_db(got2["Fft.Avg"], st.avg, what="two calls Fft.Avg")


@pytest.mark.parametrize("n", [4096, 1048576])
def test_chunked_batch_equals_one_launch_bit_for_bit(ksa, torch_cuda, n):
    """Only the chunking differs: a one-tap engine with all-ones taps folds y = x exactly (fmaf(x, 1, 0)) and hands the transform
    stage the shape of an AVG engine with one rectangular window per frame (full_size = N) and the same mag_scale -- but runs
    its batch of chunk + 5 frames as two fold + transform chunks on the shipped KSA_PFB_CHUNK_BYTES, where the AVG engine runs
    one launch.  ksa_frames_dev in one call each: per-frame dB rows, per-frame waterfall rows, Cur, Max, Min, AVG, the ring
    (N = 4096: 8197 frames wrap it 64 times, the last rows come from both chunks) and hm_index must be the same bits."""
    torch = torch_cuda
    xres, frames = 64, chunk_frames(n) + 5
    dev = _dev(torch, _stream(frames * n, seed=23))
    mk = {"pfb": dict(pfb_taps=1, window=np.ones(n)), "avg": dict(full_size=n, non_overlap=1.0, window="ones", cumu_mode="AVG")}
    res = {}
    for name, shape in mk.items():
        eng = ksa.SpectrumEngine(n, gain=GAIN, xres=xres, max_frames=frames, **shape)
        db = torch.full((frames, n), -1.0, dtype=torch.float32, device="cuda")
        rows = torch.full((frames, xres), -1.0, dtype=torch.float32, device="cuda")
        eng.frames_dev(dev, ksa.FMT_C64, frames, cur_db=db, hm_rows=rows, frame_stride=n)
        eng.synchronize()
        res[name] = (eng.mag_scale, eng.kernel_info(), eng.state(), db, rows)
        eng.close()
    a, b = res["pfb"], res["avg"]
    assert a[0] == b[0] and a[1] == b[1]
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])
    for k in CURVES + ("fftHM",):
        assert np.array_equal(a[2][k], b[2][k]), k
    assert a[2]["hm_index"] == b[2]["hm_index"] == frames % 128 and a[2]["frames"] == frames


def test_chunked_state_against_the_model(ksa, torch_cuda):
    """N = 2^20, P = 2, three frames more than one chunk through ksa_frames_dev at stride N: the frames either side of the chunk
    boundary, the first and the last against the model -- per-frame dB rows, per-frame waterfall rows, the ring rows they went
    to, Cur."""
    torch = torch_cuda
    n, p, xres = 1048576, 2, 64
    frames = chunk_frames(n) + 3
    assert frames < 128
    x = _stream((frames - 1 + p) * n, seed=29)
    eng = ksa.SpectrumEngine(n, pfb_taps=p, window="hanning", gain=GAIN, xres=xres, max_frames=frames)
    db = torch.full((frames, n), -1.0, dtype=torch.float32, device="cuda")
    rows = torch.full((frames, xres), -1.0, dtype=torch.float32, device="cuda")
    eng.frames_dev(_dev(torch, x), ksa.FMT_C64, frames, cur_db=db, hm_rows=rows, frame_stride=n)
    eng.synchronize()
    got = eng.state()
    taps = eng.win
    eng.close()
    assert got["hm_index"] == frames and got["frames"] == frames
    rows = rows.cpu().numpy()
    for f in (0, chunk_frames(n) - 1, chunk_frames(n), frames - 1):
        want = orc.log_no_gain(pfb.spectrum(x[f * n:(f + p) * n], n, taps), GAIN)
        assert_db(db[f].cpu().numpy(), want, what="frame %d dB" % f)
        assert_db(rows[f], orc.plotcompress(want, xres, "MAX"), what="frame %d row" % f)
        assert np.array_equal(got["fftHM"][f], rows[f].astype(np.float64)), "ring row %d" % f
    assert np.array_equal(got["Fft.Cur"], db[frames - 1].cpu().numpy().astype(np.float64))


@pytest.mark.parametrize("n,p,frames", [(512, 4, 40), (4096, 4, 300)])
def test_host_batches_equal_frames_dev_on_a_device_copy(ksa, torch_cuda, n, p, frames):
    """SpectrumEngine.frames from numpy blocks [k][P*N], complex64 and uint8, against frames_dev on a device copy of the same
    blocks: state, per-frame spectra and rows bit for bit (300 blocks of 128 KiB cross PCIe in two slots)."""
    torch = torch_cuda
    xres = 64
    x = _stream(frames * p * n, seed=13).reshape(frames, p * n)
    raw = orc.quantize_u8(x.reshape(-1)).reshape(frames, 2 * p * n)
    for fmt, blocks in ((ksa.FMT_C64, x), (ksa.FMT_U8, raw)):
        eng = ksa.SpectrumEngine(n, pfb_taps=p, window="hanning", gain=GAIN, xres=xres, max_frames=frames)
        hdb, hrows = eng.frames(blocks, cur_db=True, hm_rows=True)
        host = eng.state()
        eng.reset()
        db = torch.empty((frames, n), dtype=torch.float32, device="cuda")
        rows = torch.empty((frames, xres), dtype=torch.float32, device="cuda")
        eng.frames_dev(_dev(torch, blocks.reshape(-1)), fmt, frames, cur_db=db, hm_rows=rows)
        eng.synchronize()
        dev = eng.state()
        eng.close()
        assert np.array_equal(hdb, db.cpu().numpy()) and np.array_equal(hrows, rows.cpu().numpy()), fmt
        for k in CURVES + ("fftHM",):
            assert np.array_equal(host[k], dev[k]), (fmt, k)
        assert host["hm_index"] == dev["hm_index"] == frames % 128
        if fmt == ksa.FMT_C64:
            assert_db(hdb[-1], orc.log_no_gain(pfb.spectrum(x[-1], n, pfb.prototype(n, p, "hanning")), GAIN), what="last block")


def test_scan_pass_against_the_oracle_stitch(ksa, torch_cuda):
    """One pass over three bands (N = 512, P = 4): ksa_scan_pass_c64, ksa_scan_pass_dev and ksa_scan_pass_u8 against ScanState
    fed with the model's spectra."""
    torch = torch_cuda
    n, p, xres, min_amp = 512, 4, 128, (1 / 256) * 0.00001
    geo = dict(start_freq=100e6, end_freq=107.2e6, sampling_rate=2.4e6)
    taps = pfb.prototype(n, p, "hamming")

    def reference(blocks):
        st = orc.ScanState(n, geo["start_freq"], geo["end_freq"], geo["sampling_rate"], GAIN, min_amp, xres, 0.5)
        st.run_pass([pfb.spectrum(b, n, taps) for b in blocks])
        return st
    steps = len(reference([]).centers)
    x = _stream(steps * p * n, seed=17).reshape(steps, p * n)
    raw = orc.quantize_u8(x.reshape(-1)).reshape(steps, 2 * p * n)
    st, st8 = reference(x), reference(orc.unpack_u8(raw.reshape(-1)).reshape(steps, p * n))
    assert st.num_groups == 3
    eng = ksa.SpectrumEngine(n, pfb_taps=p, window="hamming", gain=GAIN, min_amp=min_amp, xres=xres, max_frames=steps, scan_total_entries=st.total,
                             scan_non_overlap=0.5)

    def check(ref, what):
        got = eng.scan_state()
        top = 10 ** (np.max(ref.max) / 10)
        for k in ("cur", "max", "min", "avg"):
            assert_db(got["Fft." + k.capitalize()], getattr(ref, k), what="%s %s" % (what, k), top=top)
        assert_db(got["fftHM"], ref.hm, what=what + " ring", top=top)
        assert got["hm_index"] == 1 and got["passes"] == 1
    eng.scan_pass(x)
    check(st, "scan_pass_c64")
    eng.scan_reset()
    eng.scan_pass_dev(_dev(torch, x.reshape(-1)), ksa.FMT_C64, steps)
    eng.synchronize()
    check(st, "scan_pass_dev")
    eng.scan_reset()
    eng.scan_pass(raw)
    check(st8, "scan_pass_u8")
    eng.close()


def test_front_end_zerospan_with_pfb_taps(ksa):
    """`zeroSpan fftSize 512 pfbTaps 4 window hanning source synth prgLoopCnt 8`: Fft.Cur is the model of the last block the
    synthetic source delivered (a second source with the same seed replays the reads: the 16Ki settle read, then 8 blocks)."""
    load_pkg()
    K = importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")
    sources = importlib.import_module("prgs-sdr-kspecanal_amd.sources")
    d = K.main(["zeroSpan", "fftSize", "512", "pfbTaps", "4", "window", "hanning", "source", "synth", "prgLoopCnt", "8",
                "bPltLevels", "false", "bPltHeatMap", "false"])
    assert d["fullSize"] == 2048 and d["fftHMIndex"] == 8
    src = sources.SyntheticSdr()
    src.sample_rate, src.center_freq, src.gain = d["samplingRate"], d["centerFreq"], d["gain"]
    src.read_samples(16 * 1024)
    for _ in range(8):
        last = np.asarray(src.read_samples(2048)).astype(np.complex64)
    want = pfb.spectrum(last, 512, pfb.prototype(512, 4, "hanning"))
    assert_db(d["Fft.Cur"], orc.log_no_gain(want, d["gain"]), what="front end Fft.Cur")
