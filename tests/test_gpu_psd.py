"""GPU tests of the Welch PSD fold (cumu_mode PSD, curScanCumuMode psd): every kernel path and both sample formats against the
float64 restatement (psd_helper.py), the reference-run psd_* fixtures, dB units, zero / NaN blocks, zeroSpan through the device
and host batch entries (commit and merge routes), the scan entries, and the front end.

Tolerances are the project's own: linear results as AMPLITUDES sqrt(P) with assert_lin at 1e-5 of the strongest bin (1e-5 of
the strongest power would leave everything more than 50 dB down unchecked), dB results with assert_db as it stands."""
import importlib

import numpy as np
import pytest

import ksa_oracle as orc
import psd_helper as ph
from conftest import golden, load_pkg
from test_gpu_parity import assert_lin, assert_db, GAIN

pytestmark = pytest.mark.gpu
CURVES = ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def assert_psd(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.all(got >= 0), what + ": negative power"
    assert_lin(np.sqrt(got), np.sqrt(want), what=what)


def _xres(n):
    """A waterfall width that divides N (curscan_dev writes no waterfall; the engine still wants a valid one)."""
    return n if n & (n - 1) else min(n, 512)


def _dev(torch, ksa, x, fmt):
    if fmt == ksa.FMT_U8:
        return torch.from_numpy(x).to("cuda")
    return torch.view_as_real(torch.from_numpy(x)).to("cuda")


# (N, fullSize, nonOverlap, window, frames, path reported by kernel_info, what the case is there for)
# frames: an int, or "pair" / "fill": as many frames as the pair kernel (path 4) or an unsplit launch needs, spaced `stride` apart
PATHS = [
    (16, 128, 0.1, "ones", 3, 0, "M = 1"),
    (32, 256, 0.25, "hanning", 3, 0, "two passes"),
    (64, 512, 0.1, "ones", 5, 5, "8 x 8 plan, rectangular window; uint8 runs spectrum_kernel<64>"),
    (64, 4160, 0.1, "hamming", 3, 5, "8 x 8 plan with taps, 650 windows"),
    (64, 512, 0.5, "hanning", 4, 5, "8 x 8 plan, 50 % overlap"),
    (64, 512, 0.25, "kaiser", 4, 5, "8 x 8 plan, 75 % overlap"),
    (64, 512, 1.0, "ones", 4, 5, "8 x 8 plan, no overlap"),
    (128, 1024, 1.0, "kaiser", 3, 0, "no overlap"),
    (256, 2048, 0.25, "hamming", 4, 0, "slots"),
    (512, 4096, 0.5, "kaiser", 3, 0, "one transform per workgroup"),
    (1024, 8192, 0.5, "kaiser", 3, 4, "small batch: spectrum_kernel<1024, RM 8>, window split"),
    (1024, 2048, 0.5, "hanning", "pair", 4, "pair kernel RM 8"),
    (1024, 3072, 0.25, "hamming", "pair", 4, "pair kernel RM 4"),
    (1024, 2048, 0.1, "ones", "pair", 4, "pair kernel RM 0"),
    (1024, 2048, 1.0, "kaiser", "pair", 4, "pair kernel, no overlap"),
    (2048, 16384, 0.25, "hanning", 2, 0, "RM 4, window split"),
    (4096, 32768, 0.5, "hanning", 1, 0, "ping-pong form, window split (one-frame batch)"),
    (4096, 8192, 0.5, "hanning", "fill", 0, "ping-pong form, unsplit"),
    (4096, 8192, 0.1, "kaiser", "fill", 0, "rolled loop, fractional hops (constant fold where the other folds branch)"),
    (4096, 32768, 0.25, "ones", 2, 0, "RM 4"),
    (8192, 65536, 0.5, "hanning", 2, 3, "32 points per thread, window split"),
    (8192, 16384, 0.25, "hamming", "fill", 3, "32 points per thread, unsplit"),
    (8192, 32768, 1.0, "ones", "fill", 3, "32 points per thread, no overlap, rectangular window"),
    (16384, 131072, 0.1, "kaiser", 1, 3, "32 points per thread, window split"),
    (16384, 32768, 0.25, "hanning", "fill", 3, "32 points per thread, unsplit"),
    (32768, 65536, 0.5, "hamming", 2, 2, "radix-16 first stage"),
    (65536, 131072, 0.25, "hanning", 1, 2, "radix-16 first stage, 4096-point second stage"),
    (524288, 1048576, 0.5, "kaiser", 1, 2, "radix-32 first stage"),
    (1048576, 2097152, 1.0, "hanning", 1, 2, "radix-64 first stage"),
    (20, 160, 0.1, "ones", 3, 6, "mixed radix 4 * 5"),
    (1000, 8000, 0.5, "hanning", 3, 6, "mixed radix"),
    (1000, 8000, 1.0, "hamming", 3, 6, "mixed radix, no overlap"),
    (240, 1920, 0.25, "ones", 3, 6, "mixed radix, 75 % overlap"),
    (2400, 19200, 0.1, "kaiser", 2, 6, "mixed radix"),
    (16200, 32400, 0.25, "hamming", 2, 6, "mixed radix, the largest plan"),
]


@pytest.mark.parametrize("case", PATHS, ids=["%d-%s-%s-%s" % (c[0], c[2], c[3], c[4]) for c in PATHS])
def test_curscan_dev_linear_on_every_path(ksa, torch_cuda, case):
    torch = torch_cuda
    n, full, q, window, frames, path, _ = case
    win = orc.window_table(window, n)
    probe = ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window=window, cumu_mode="PSD", xres=_xres(n))
    info = probe.kernel_info()
    probe.close()
    assert info["path"] == path, info
    stride = full
    if frames == "pair":          # the pair kernel takes batches of at least two pairs per resident workgroup
        frames, stride = 2 * info["grid"] + 1, 64
    elif frames == "fill":        # more frames than half the resident workgroups: no window split
        frames, stride = info["grid"] // 2 + 3, 512
    total = (frames - 1) * stride + full
    x = (orc.synth_iq(total, 7000 + n + frames) * 0.7).astype(np.complex64)
    raw = orc.quantize_u8(x)
    eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window=window, cumu_mode="PSD", xres=_xres(n), max_frames=frames)
    assert np.array_equal(eng.starts, ph.geometry(full, n, q)[2]) and eng.mag_scale == ph.scale(win, len(eng.starts))
    out = torch.empty((frames, n), dtype=torch.float32, device="cuda")
    check = sorted(set(np.linspace(0, frames - 1, min(frames, 12)).astype(int)))
    for fmt, src, ref_in in ((ksa.FMT_C64, x, x), (ksa.FMT_U8, raw, orc.unpack_u8(raw))):
        out.fill_(-1.0)
        eng.curscan_dev(_dev(torch, ksa, src, fmt), fmt, frames, out, frame_stride=stride)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for f in check:
            want = ph.psd(ref_in[f * stride:f * stride + full], n, q, win)
            assert_psd(got[f], want, what="N=%d q=%s %s fmt %d frame %d/%d" % (n, q, window, fmt, f, frames))
    eng.close()


@pytest.mark.parametrize("n", [64, 512, 2400, 4096])
def test_reference_fixtures_through_host_pointer_and_batch(ksa, torch_cuda, n):
    """The reference's own bUsePSD results: through SpectrumEngine.curscan (host pointer, a one-frame batch: the window-split
    mode from N = 1024 up) and through a device batch of the same block repeated; both against the fixture and each other."""
    torch = torch_cuda
    g = golden("psd_curscan_n%d" % n)
    full = int(g["full"])
    x = orc.synth_iq(full, int(g["seed"])).astype(np.complex64)
    for w, q, key in ph.fixture_cases(g):
        one = ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window=w, cumu_mode="PSD", xres=_xres(n))
        host = one.curscan(x)
        one.close()
        assert_psd(host, g[key], what="%d %s %s host" % (n, w, q))
        frames = 800
        eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window=w, cumu_mode="PSD", xres=_xres(n), max_frames=frames)
        out = torch.empty((frames, n), dtype=torch.float32, device="cuda")
        eng.curscan_dev(_dev(torch, ksa, x, ksa.FMT_C64), ksa.FMT_C64, frames, out, frame_stride=0)
        torch.cuda.synchronize()
        batch = out.cpu().numpy()
        eng.close()
        assert np.array_equal(batch[0], batch[-1]) and np.array_equal(batch[0], batch[frames // 2])
        assert_psd(batch[0], g[key], what="%d %s %s batch" % (n, w, q))
        assert_psd(batch[0], host, what="%d %s %s batch against host" % (n, w, q))


def test_large_reference_fixture(ksa):
    g = golden("psd_curscan_n32768")
    n, full = int(g["fft_size"]), int(g["full"])
    x = orc.synth_iq(full, int(g["seed"])).astype(np.complex64)
    eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=float(g["non_overlap"]), window=str(g["window"]), cumu_mode="PSD")
    got = eng.curscan(x)
    eng.close()
    e = np.max(np.abs(np.sqrt(got[g["idx"]]) - np.sqrt(g["psd_at_idx"]))) / np.sqrt(float(g["peak"]))
    assert e <= 1e-5, e


@pytest.mark.parametrize("n,full,q,window", [(64, 512, 0.1, "ones"), (1024, 8192, 0.5, "hanning"), (4096, 32768, 0.5, "hanning"),
                                             (16384, 32768, 0.25, "kaiser"), (2400, 19200, 0.25, "hamming"), (32768, 65536, 0.5, "hanning")])
def test_db_units_zero_block_and_nan_sample(ksa, torch_cuda, n, full, q, window):
    """OUT_DB / OUT_DB_CLIP are LogNoGain / Clip2MinAmp on the PSD (K:109, K:101); frame 1 of the batch is all zero (-inf dB,
    and the clipped floor in scan units), frame 2 holds one NaN sample: the PSD is a mean, so every bin of that frame is NaN."""
    torch = torch_cuda
    min_amp = 2e-3      # inside the range of the PSD's bins, so that the clip bites
    win = orc.window_table(window, n)
    x = (orc.synth_iq(3 * full, 5 + n) * 0.7).astype(np.complex64).reshape(3, full)
    x[1] = 0
    x[2, full // 2 + 3] = np.nan
    want = ph.psd(x[0], n, q, win)
    for fmt in (ksa.FMT_C64, ksa.FMT_U8):
        if fmt == ksa.FMT_U8:
            src = orc.quantize_u8(x[:2].reshape(-1))            # (uint8 samples hold no NaN and no exact zero level)
            ref = ph.psd(orc.unpack_u8(src[:2 * full]), n, q, win)
            frames = 1
        else:
            src, ref, frames = x.reshape(-1), want, 3
        eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window=window, cumu_mode="PSD", gain=GAIN, min_amp=min_amp,
                                 xres=_xres(n), max_frames=3)
        dev = _dev(torch, ksa, src, fmt)
        out = torch.empty((frames, n), dtype=torch.float32, device="cuda")
        eng.curscan_dev(dev, fmt, frames, out, out_mode=ksa.OUT_DB)
        torch.cuda.synchronize()
        db = out.cpu().numpy()
        assert_db(db[0], orc.log_no_gain(np.copy(ref), GAIN), what="%d OUT_DB fmt %d" % (n, fmt))
        eng.curscan_dev(dev, fmt, frames, out, out_mode=ksa.OUT_DB_CLIP)
        torch.cuda.synchronize()
        clip = out.cpu().numpy()
        assert np.sum(ref < min_amp) > 0
        assert_db(clip[0], orc.log_no_gain(orc.clip2minamp(np.copy(ref), min_amp), GAIN, inf_to=0), what="%d OUT_DB_CLIP fmt %d" % (n, fmt))
        if frames == 3:
            floor = 10 * np.log10(min_amp) - GAIN
            assert np.all(np.isneginf(db[1])) and np.allclose(clip[1], floor, atol=1e-4)
            assert np.all(np.isnan(db[2])) and np.all(np.isnan(clip[2]))
            eng.curscan_dev(dev, fmt, frames, out, out_mode=ksa.OUT_LINEAR)
            torch.cuda.synchronize()
            lin = out.cpu().numpy()
            assert np.all(lin[1] == 0) and np.all(np.isnan(lin[2]))
        eng.close()
    # minAmp4Clip 0: the zero block's -inf becomes 0 in scan units (infTo = 0, K:641)
    eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window=window, cumu_mode="PSD", gain=GAIN, min_amp=0.0, xres=_xres(n))
    out = torch.empty((1, n), dtype=torch.float32, device="cuda")
    eng.curscan_dev(_dev(torch, ksa, x[1], ksa.FMT_C64), ksa.FMT_C64, 1, out, out_mode=ksa.OUT_DB_CLIP)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 0)
    eng.close()


def _check_state(got, st, what, frames):
    for k in CURVES:
        assert_db(got[k], getattr(st, k[4:].lower()), what="%s %s" % (what, k))
    assert_db(got["fftHM"], st.hm, what=what + " ring")
    assert got["hm_index"] == frames % 128 and got["frames"] == frames


@pytest.mark.parametrize("n,full,q,window,xres", [(512, 4096, 0.5, "hanning", 128), (1024, 2048, 0.25, "kaiser", 256),
                                                  (2400, 4800, 0.5, "hamming", 300)])
def test_zerospan_batches_against_the_oracle_state(ksa, torch_cuda, n, full, q, window, xres):
    """260 frames (the ring wraps): ksa_frames_dev, ksa_frames_c64 and ksa_frames_u8 with commit = 1, and two halves with
    commit = 0 merged by ksa_allreduce_state, against ZeroSpanState fed with restated PSDs: curves, per-frame dB rows,
    per-frame waterfall rows, ring."""
    torch = torch_cuda
    frames = 260
    win = orc.window_table(window, n)
    x = (orc.synth_iq(full * frames, 321 + n) * 0.7).astype(np.complex64).reshape(frames, full)
    raw = orc.quantize_u8(x.reshape(-1)).reshape(frames, 2 * full)
    mk = lambda mf: ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window=window, cumu_mode="PSD", gain=GAIN, xres=xres,
                                       max_frames=mf)

    def reference(blocks):
        st = orc.ZeroSpanState(n, xres, GAIN)
        db = np.array([st.push(ph.psd(b, n, q, win)) for b in blocks])
        return st, db
    st, db_ref = reference(x)
    rows_ref = np.array([orc.plotcompress(r, xres, "MAX") for r in db_ref])
    # device batch
    eng = mk(frames)
    db = torch.empty((frames, n), dtype=torch.float32, device="cuda")
    rows = torch.empty((frames, eng.hm_width), dtype=torch.float32, device="cuda")
    eng.frames_dev(_dev(torch, ksa, x.reshape(-1), ksa.FMT_C64), ksa.FMT_C64, frames, cur_db=db, hm_rows=rows)
    eng.synchronize()
    _check_state(eng.state(), st, "frames_dev", frames)
    assert_db(db.cpu().numpy(), db_ref, what="frames_dev per-frame dB")
    assert_db(rows.cpu().numpy(), rows_ref, what="frames_dev rows")
    # host batch, complex64
    eng.reset()
    hdb, hrows = eng.frames(x, cur_db=True, hm_rows=True)
    _check_state(eng.state(), st, "ksa_frames_c64", frames)
    assert_db(hdb, db_ref, what="ksa_frames_c64 per-frame dB")
    assert_db(hrows, rows_ref, what="ksa_frames_c64 rows")
    eng.close()
    # host batch, uint8
    st8, db8 = reference(orc.unpack_u8(raw.reshape(-1)).reshape(frames, full))
    eng = mk(frames)
    hdb, _ = eng.frames(raw, cur_db=True)
    _check_state(eng.state(), st8, "ksa_frames_u8", frames)
    assert_db(hdb, db8, what="ksa_frames_u8 per-frame dB")
    eng.close()
    # commit = 0 and the merge route: two engines, half of the run each
    half = frames // 2
    pair = [mk(half), mk(half)]
    for r in range(2):
        pair[r].set_hm_index((r * half) % 128)
        pair[r].frames(x[r * half:(r + 1) * half], first_index=r * half, total_frames=frames, commit=False)
    ksa.allreduce_state(pair, half)
    for r in range(2):
        _check_state(pair[r].state(), st, "merged rank %d" % r, frames)
        pair[r].close()


def test_zerospan_fixture_end_to_end(ksa):
    g = golden("psd_zerospan_n512")
    n, q, full, frames = int(g["fft_size"]), float(g["non_overlap"]), int(g["full"]), int(g["frames"])
    x = orc.synth_iq(full * frames, int(g["seed"])).astype(np.complex64).reshape(frames, full)
    mk = lambda mf: ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window=str(g["window"]), cumu_mode="PSD",
                                       gain=float(g["gain"]), xres=int(g["xres"]), max_frames=mf)
    batch, loop = mk(frames), mk(1)
    batch.frames(x)
    for f in x:
        loop.frame(f)
    for eng, what in ((batch, "ksa_frames_c64"), (loop, "ksa_frame_c64 loop")):
        got = eng.state()
        for k in CURVES:
            assert_db(got[k], g[k[4:].lower()], what="%s %s" % (what, k))
        assert_db(got["fftHM"][:frames], g["hm"][:frames], what=what + " ring")
        assert got["hm_index"] == frames % 128
        eng.close()


def test_scan_entries_against_the_fixture_and_the_oracle_state(ksa, torch_cuda):
    """ksa_scan_pass_c64 pass by pass and ksa_scan_passes_dev in one call: the reference's bUsePSD scan (three bands, 69 segments
    per block) and ScanState fed with restated PSDs; ksa_scan_pass_u8 against ScanState on the unpacked samples."""
    torch = torch_cuda
    g = golden("psd_scan_3band_n512")
    n, full, passes, steps = int(g["fft_size"]), int(g["full"]), int(g["passes"]), int(g["steps"])
    st, x = ph.scan_state(g)
    x = x.reshape(passes, steps, full)
    mk = lambda: ksa.SpectrumEngine(n, full_size=full, non_overlap=float(g["non_overlap"]), window=str(g["window"]), cumu_mode="PSD",
                                    gain=float(g["gain"]), min_amp=float(g["min_amp"]), xres=int(g["xres"]), max_frames=steps * passes,
                                    scan_total_entries=st.total, scan_non_overlap=float(g["scan_non_overlap"]))
    top = 10 ** (np.max(g["max"]) / 10)

    def check(got, ref, what):
        for k in ("cur", "max", "min", "avg"):
            assert_db(got["Fft." + k.capitalize()], ref[k] if isinstance(ref, dict) else getattr(ref, k), what="%s %s" % (what, k), top=top)
        hm = ref["hm"] if isinstance(ref, dict) else ref.hm
        assert_db(got["fftHM"], hm, what=what + " ring", top=top)
    fixture = {k: g[k] for k in ("cur", "max", "min", "avg", "hm")}
    eng = mk()
    assert len(eng.starts) == 69
    for p in range(passes):
        eng.scan_pass(x[p])
    got = eng.scan_state()
    check(got, fixture, "scan_pass_c64 fixture")
    check(got, st, "scan_pass_c64 oracle")
    assert got["hm_index"] == int(g["hm_index"]) and got["passes"] == passes
    eng.scan_reset()
    eng.scan_passes_dev(_dev(torch, ksa, x.reshape(-1), ksa.FMT_C64), ksa.FMT_C64, steps, passes)
    eng.synchronize()
    check(eng.scan_state(), fixture, "scan_passes_dev fixture")
    # uint8
    raw = orc.quantize_u8(x.reshape(-1) * 0.7)
    st8, _ = ph.scan_state(g, orc.unpack_u8(raw))
    eng.scan_reset()
    for p in range(passes):
        eng.scan_pass(raw.reshape(passes, steps, 2 * full)[p])
    check(eng.scan_state(), st8, "scan_pass_u8 oracle")
    eng.close()


# ------------------------------------------------------------------------------------------------ the front end
def _capture(tmp_path, frames, full, seed):
    x = orc.synth_iq(16 * 1024 + full * frames, seed) * 0.7
    raw = orc.quantize_u8(x)
    path = tmp_path / ("capture%d.bin" % seed)
    raw.tofile(path)
    return str(path), orc.unpack_u8(raw[2 * 16 * 1024:]).reshape(frames, full)       # sdr_setup discards 16Ki first (K:301)


@pytest.fixture()
def K():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")


def test_front_end_zerospan_psd_with_frame_batch(ksa, K, tmp_path):
    """`zeroSpan curScanCumuMode psd frameBatch 64` over a uint8 `file:` capture, both hand-over formats: Fft.* and the waterfall
    carry the PSD (ZeroSpanState fed with restated PSDs); frameBatch 1 gives the same curves."""
    n, frames, q = 1024, 150, 0.25
    full = orc.full_size(n, 2.4e6)
    path, blocks = _capture(tmp_path, frames, full, 1212)
    win = orc.window_table("hanning", n)
    st = orc.ZeroSpanState(n, 256, 19.1)
    for b in blocks:
        st.push(ph.psd(b, n, q, win))
    common = ["zeroSpan", "fftSize", str(n), "window", "hanning", "curScanNonOverlap", str(q), "curScanCumuMode", "psd", "xRes", "256",
              "bPltLevels", "false", "bPltHeatMap", "false", "source", "file:%s" % path, "prgLoopCnt", str(frames)]
    for extra in (["frameBatch", "64", "iqFormat", "c64"], ["frameBatch", "64", "iqFormat", "u8"], ["frameBatch", "1", "iqFormat", "u8"]):
        d = K.main(common + extra)
        for k in CURVES:
            assert_db(d[k], getattr(st, k[4:].lower()), what="front end %s %s" % (extra, k))
        assert_db(d["fftHM"], st.hm, what="front end %s waterfall" % extra)
        assert d["fftHMIndex"] == frames % 128


def test_front_end_psd_with_the_host_diagnostic(ksa, K, tmp_path, capsys):
    """`curScanCumuMode psd bUsePSD true`: the diagnostic compares like with like -- d['psd.cur'] is matplotlib's linear,
    fftshifted pxx of the last block and 10*log10(pxx) - gain is Fft.Cur; the peak bins and levels of psd.check agree."""
    n, frames, q = 2048, 3, 0.5
    full = orc.full_size(n, 2.4e6)
    path, blocks = _capture(tmp_path, frames, full, 1313)
    d = K.main(["zeroSpan", "fftSize", str(n), "window", "kaiser", "curScanNonOverlap", str(q), "curScanCumuMode", "psd",
                "bUsePSD", "true", "bPltLevels", "false", "bPltHeatMap", "false", "source", "file:%s" % path, "prgLoopCnt", str(frames)])
    assert "DBUG:bUsePSD" in capsys.readouterr().out
    assert_psd(d["psd.cur"], ph.psd(blocks[-1], n, q, orc.window_table("kaiser", n)), what="psd.cur")
    assert_db(d["Fft.Cur"], 10 * np.log10(d["psd.cur"]) - d["gain"], what="Fft.Cur against the diagnostic")
    kg, kp, lg, lp = d["psd.check"]
    assert kg == kp and abs(lg - lp) <= 5e-3


def test_front_end_scan_psd_on_the_reference_stream(ksa, K):
    """`scan ... curScanCumuMode psd` fed with the stream the reference consumed under bUsePSD true: the stitched curves and the
    waterfall against the reference's own."""
    g = golden("psd_scan_3band_n512")
    n, full, passes, steps = int(g["fft_size"]), int(g["full"]), int(g["passes"]), int(g["steps"])
    stream = orc.synth_iq(full * steps * passes, int(g["seed"])).astype(np.complex64)

    class Replay:
        valid_gains_db, bandwidth, freq_correction = [19.1], 0, 0
        pos = 0

        def __init__(self):
            self.sample_rate = self.center_freq = 0
            self._gain, self._settle = 0, False

        gain = property(lambda self: self._gain)

        @gain.setter
        def gain(self, v):
            self._gain, self._settle = v, True

        def read_samples(self, cnt):
            cnt = int(cnt)
            if self._settle:                      # the 16Ki settle read after a retune (K:301) is discarded
                self._settle = False
                return np.zeros(cnt, dtype=np.complex64)
            out = stream[Replay.pos:Replay.pos + cnt]
            Replay.pos += cnt
            return out

        def close(self):
            pass
    orig = K.open_source
    K.open_source = lambda d: Replay()
    try:
        d = K.main(["scan", "startFreq", "100e6", "endFreq", "107.2e6", "fftSize", str(n), "window", "kaiser", "curScanCumuMode", "psd",
                    "prgLoopCnt", str(passes), "bPltLevels", "false", "bPltHeatMap", "false"])
    finally:
        K.open_source = orig
    assert Replay.pos == len(stream)
    top = 10 ** (np.max(g["max"]) / 10)
    for k in ("cur", "max", "min", "avg"):
        assert_db(d["Fft." + k.capitalize()], g[k], what="scan main " + k, top=top)
    assert_db(d["fftHM"], g["hm"], what="scan main waterfall", top=top)
