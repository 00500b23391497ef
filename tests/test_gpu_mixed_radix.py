"""GPU tests of the mixed-radix path (path 6): fftSize N = 2^a*3^b*5^c, a multiple of 4, 16..16384, not a power of two.
Every such N against the oracle, fold modes x windows x output units against the reference-run mr_* fixtures, NaN / zero
blocks, zeroSpan (device batch, host batches, per-frame loop) and a scan at N = 2400, the kernel report and the refusals."""
import ctypes as C

import numpy as np
import pytest

import ksa_oracle as orc
from conftest import golden
from test_gpu_parity import assert_lin, assert_db, GAIN

pytestmark = pytest.mark.gpu
WINDOWS = ("ones", "hanning", "hamming", "kaiser")
MODES = ("AVG", "MAX", "MIN", "RAW")
CURVES = ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg")


def _mixed():
    out = []
    for n in range(20, 16385, 4):
        m = n
        for f in (2, 3, 5):
            while m % f == 0:
                m //= f
        if m == 1 and n & (n - 1):
            out.append(n)
    return out


MIXED = _mixed()


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def test_every_mixed_size_against_the_oracle(ksa, torch_cuda):
    """All 123 sizes, complex64 and uint8 input, hanning, AVG, linear: curscan_dev against oracle.curscan."""
    torch = torch_cuda
    assert len(MIXED) == 123
    for n in MIXED:
        full = 2 * n
        x = (orc.synth_iq(full, 9000 + n) * 0.7).astype(np.complex64)
        raw = orc.quantize_u8(x)
        win = orc.window_table("hanning", n)
        eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=0.25, window="hanning", xres=n, max_frames=1)
        info = eng.kernel_info()
        assert info["path"] == 6 and info["lds_bytes"] == 8 * n and 64 <= info["threads"] <= 1024, (n, info)
        out = torch.empty(n, dtype=torch.float32, device="cuda")
        for fmt, src, ref_in in ((ksa.FMT_C64, torch.view_as_real(torch.from_numpy(x)), x),
                                 (ksa.FMT_U8, torch.from_numpy(raw), orc.unpack_u8(raw))):
            eng.curscan_dev(src.to("cuda"), fmt, 1, out)
            torch.cuda.synchronize()
            assert_lin(out.cpu().numpy(), orc.curscan(ref_in, n, 0.25, win, "AVG"), what="N=%d fmt %d" % (n, fmt))
        eng.close()


@pytest.mark.parametrize("n", [20, 96, 240, 1000, 2400])
def test_folds_windows_and_units_against_the_reference(ksa, torch_cuda, n):
    torch = torch_cuda
    g = golden("mr_curscan_n%d" % n)
    x, q, full = g["iq"], float(g["non_overlap"]), int(g["full"])
    dev = torch.view_as_real(torch.from_numpy(x)).to("cuda")
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    min_amp = ksa.engine.MIN_AMP_DEFAULT
    for window in WINDOWS:
        for mode in MODES:
            want = g["%s_%s" % (window, mode)]
            eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window=window, cumu_mode=mode, gain=GAIN, xres=n)
            assert_lin(eng.curscan(x), want, what="%d %s %s host" % (n, window, mode))
            for unit, ref in ((ksa.OUT_DB, orc.log_no_gain(np.copy(want), GAIN)),
                              (ksa.OUT_DB_CLIP, orc.log_no_gain(orc.clip2minamp(np.copy(want), min_amp), GAIN, inf_to=0))):
                eng.curscan_dev(dev, ksa.FMT_C64, 1, out, out_mode=unit)
                torch.cuda.synchronize()
                assert_db(out.cpu().numpy(), ref, what="%d %s %s unit %d" % (n, window, mode, unit))
            eng.close()


@pytest.mark.parametrize("n", [12000, 15360])
def test_large_sizes_against_the_reference(ksa, n):
    g = golden("mr_curscan_n%d" % n)
    x = orc.synth_iq(int(g["full"]), int(g["seed"])).astype(np.complex64)
    for mode, key in (("AVG", "avg_at_idx"), ("MAX", "max_at_idx")):
        eng = ksa.SpectrumEngine(n, full_size=int(g["full"]), non_overlap=float(g["non_overlap"]), window=str(g["window"]),
                                 cumu_mode=mode, xres=n)
        got = eng.curscan(x)
        e = np.max(np.abs(got[g["idx"]] - g[key])) / float(g["peak"])
        assert e <= 1e-5, (n, mode, e)
        eng.close()


@pytest.mark.parametrize("n", [240, 2400])
def test_zero_block_and_nan_sample(ksa, n):
    """A zero block gives -inf dB; a NaN sample keeps the bins it reaches NaN under MAX and MIN (np.max / np.min, K:141-143)."""
    full = 4 * n
    eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=0.5, window="hanning", max_frames=1, xres=n // 4)
    eng.frame(np.zeros(full, dtype=np.complex64))
    st = eng.state()
    assert np.all(np.isneginf(st["Fft.Cur"])) and np.all(np.isneginf(st["Fft.Avg"]))
    eng.close()
    x = orc.synth_iq(full, 77).astype(np.complex64)
    x[n // 3] = np.nan
    win = orc.window_table("hanning", n)
    for mode in ("MAX", "MIN"):
        eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=0.5, window="hanning", cumu_mode=mode, xres=n)
        got = eng.curscan(x)
        want = orc.curscan(x, n, 0.5, win, mode)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).any(), mode
        ok = ~np.isnan(want)
        if ok.any():
            assert_lin(got[ok], want[ok], what="NaN " + mode)
        eng.close()


def _zs_fixture():
    g = golden("mr_zerospan_n2400")
    n, q, full, frames = int(g["fft_size"]), float(g["non_overlap"]), int(g["full"]), int(g["frames"])
    x = orc.synth_iq(full * frames, int(g["seed"])).astype(np.complex64).reshape(frames, full)
    return g, n, q, full, frames, x


def _check_state(st, g, what):
    for k in CURVES:
        assert_db(st[k], g[k[4:].lower()], what="%s %s" % (what, k))
    assert_db(st["fftHM"], g["hm"], what=what + " ring")
    assert st["hm_index"] == int(g["frames"]) % 128


def test_zerospan_2400_device_batch_and_host_batches(ksa, torch_cuda):
    """260 frames, xRes 300 (g = 8): frames_dev, ksa_frames_c64 and _u8 against the reference run; ksa_frames_c64 against the
    per-frame loop of ksa_frame_c64."""
    torch = torch_cuda
    g, n, q, full, frames, x = _zs_fixture()
    mk = lambda mf: ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window="hanning", gain=float(g["gain"]),
                                       xres=int(g["xres"]), max_frames=mf)
    eng = mk(frames)
    assert eng.hm_width == 300 and eng.kernel_info()["path"] == 6
    eng.frames_dev(torch.view_as_real(torch.from_numpy(x)).to("cuda"), ksa.FMT_C64, frames)
    eng.synchronize()
    _check_state(eng.state(), g, "frames_dev")
    eng.reset()
    eng.frames(x)
    batch = eng.state()
    _check_state(batch, g, "ksa_frames_c64")
    eng.close()
    one = mk(1)
    for f in range(frames):
        one.frame(x[f])
    loop = one.state()
    one.close()
    # Cur, Max, Min and the ring bit for bit; Avg is the same weighted sum, summed in chunks of frames by the batch and frame by
    # frame by the loop, so only its rounding may differ
    for k in ("Fft.Cur", "Fft.Max", "Fft.Min", "fftHM"):
        assert np.array_equal(batch[k], loop[k], equal_nan=True), k
    assert_db(loop["Fft.Avg"], batch["Fft.Avg"], what="loop Avg")
    assert batch["hm_index"] == loop["hm_index"] and batch["frames"] == loop["frames"]
    # uint8 input against the oracle on the unpacked samples
    raw = orc.quantize_u8(x.reshape(-1)).reshape(frames, 2 * full)
    st, db_ref, _ = orc.zerospan_batch(orc.unpack_u8(raw.reshape(-1)).reshape(frames, full), n, q,
                                       orc.window_table("hanning", n), "AVG", float(g["gain"]), 300)
    eng = mk(frames)
    db, rows = eng.frames(raw, cur_db=True, hm_rows=True)
    got = eng.state()
    for k in CURVES:
        assert_db(got[k], getattr(st, k[4:].lower()), what="u8 " + k)
    assert_db(db, db_ref, what="u8 per-frame dB")
    assert_db(rows, np.array([orc.plotcompress(r, 300, "MAX") for r in db_ref]), what="u8 rows")
    assert_db(got["fftHM"], st.hm, what="u8 ring")
    eng.close()


@pytest.mark.parametrize("n,xres", [(12000, 300), (6000, 75), (1200, 1)])
def test_zerospan_wide_waterfall_cells(ksa, torch_cuda, n, xres):
    """Cells of g = 40, 80 and 1200 bins (not powers of two) against the oracle, over the ring's wrap."""
    torch = torch_cuda
    full, q, frames = 2 * n, 0.5, 140
    x = orc.synth_iq(full * frames, 31 + n).astype(np.complex64).reshape(frames, full)
    st, db_ref, _ = orc.zerospan_batch(x, n, q, orc.window_table("kaiser", n), "AVG", GAIN, xres)
    eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window="kaiser", gain=GAIN, xres=xres, max_frames=frames)
    db = torch.empty((frames, n), dtype=torch.float32, device="cuda")
    rows = torch.empty((frames, xres), dtype=torch.float32, device="cuda")
    eng.frames_dev(torch.view_as_real(torch.from_numpy(x)).to("cuda"), ksa.FMT_C64, frames, cur_db=db, hm_rows=rows)
    eng.synchronize()
    got = eng.state()
    for k in CURVES:
        assert_db(got[k], getattr(st, k[4:].lower()), what="%d %s" % (n, k))
    assert_db(rows.cpu().numpy(), np.array([orc.plotcompress(r, xres, "MAX") for r in db_ref]), what="%d rows" % n)
    assert_db(got["fftHM"], st.hm, what="%d ring" % n)
    eng.close()


def test_scan_2400_against_the_reference(ksa):
    g = golden("mr_scan_3band_n2400")
    n, full, passes, steps = int(g["fft_size"]), int(g["full"]), int(g["passes"]), int(g["steps"])
    x = orc.synth_iq(full * steps * passes, int(g["seed"])).astype(np.complex64).reshape(passes, steps, full)
    st = orc.ScanState(n, float(g["start_freq"]), float(g["end_freq"]), float(g["sampling_rate"]), float(g["gain"]),
                       float(g["min_amp"]), int(g["xres"]), float(g["scan_non_overlap"]))
    eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=float(g["non_overlap"]), window=str(g["window"]),
                             gain=float(g["gain"]), min_amp=float(g["min_amp"]), xres=int(g["xres"]), max_frames=steps,
                             scan_total_entries=st.total, scan_non_overlap=float(g["scan_non_overlap"]))
    assert eng.scan_hop == 1200
    for p in range(passes):
        eng.scan_pass(x[p])
    got = eng.scan_state()
    top = 10 ** (np.max(g["max"]) / 10)
    for k in ("cur", "max", "min", "avg"):
        assert_db(got["Fft." + k.capitalize()], g[k], what="scan " + k, top=top)
    assert_db(got["fftHM"], g["hm"], what="scan ring", top=top)
    assert got["hm_index"] == int(g["hm_index"])
    eng.close()


def test_kernel_report_and_refusals(ksa):
    for n, path in ((2400, 6), (20, 6), (16200, 6), (4096, None), (2048, None)):
        eng = ksa.SpectrumEngine(n, full_size=2 * n, non_overlap=0.5, xres=n // 4)
        info = eng.kernel_info()
        if path is None:
            assert info["path"] != 6
        else:
            assert info["path"] == 6 and info["lds_bytes"] == 8 * n
            assert info["vgprs"] <= 128 and info["threads"] % 64 == 0 and info["grid"] >= 1, info
        eng.close()
    for n in (1009, 750, 24000):
        with pytest.raises(ksa.KsaError, match="2\\^a\\*3\\^b\\*5\\^c"):
            ksa.SpectrumEngine(n, xres=n)


def test_library_refuses_unsupported_sizes(ksa):
    _lib = __import__("importlib").import_module("prgs-sdr-kspecanal_amd._lib")
    win = np.ones(32768, dtype=np.float32)
    starts = np.zeros(1, dtype=np.int32)
    for n in (1009, 750, 24000):
        cfg = _lib.Config(abi_version=ksa.lib.ksa_abi_version(), device=0, fft_size=n, full_size=32768, num_windows=1,
                          window_starts=starts.ctypes.data_as(C.POINTER(C.c_int32)),
                          window=win.ctypes.data_as(C.POINTER(C.c_float)), mag_scale=1.0, cumu_mode=1, gain=0.0,
                          min_amp=1e-9, hm_width=0, max_frames=1, u8_offset=127.5, u8_scale=127.5)
        h = C.c_void_p()
        assert ksa.lib.ksa_create(C.byref(cfg), C.byref(h)) != 0 and not h.value
        msg = ksa.lib.ksa_last_error().decode()
        assert "power of two" in msg and "2^a*3^b*5^c" in msg, msg
    # hm_width must divide a mixed size (300 | 2400), and need not be a power of two there
    cfg.fft_size, cfg.hm_width = 2400, 7
    assert ksa.lib.ksa_create(C.byref(cfg), C.byref(h)) != 0 and "divide" in ksa.lib.ksa_last_error().decode()
    cfg.hm_width = 300
    assert ksa.lib.ksa_create(C.byref(cfg), C.byref(h)) == 0
    ksa.lib.ksa_destroy(h)
