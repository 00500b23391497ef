"""Host side of the demodulator (no GPU needed): the companion header and library, the binding, the models every GPU test
compares against, the helpers, the `demod` key of the command line, and the kernels' resource report."""
import ctypes as C
import importlib
import json
import os
import re
import wave

import numpy as np
import pytest

import demod_model as mm
from companion_helper import BY_MODULE, check_header_exports_binding
from conftest import GOLDEN, ROOT, load_pkg
from test_isa_regression import _asm, _kernels, _resource

PKG_DIR = os.path.join(ROOT, "prgs-sdr-kspecanal_amd")
EMU_SHAPES = [(1, 1), (1, 33), (2, 16), (5, 80), (64, 1024), (50, 4096)]
MODES = (mm.MODE_AM, mm.MODE_FM, mm.MODE_PM)


@pytest.fixture(scope="module")
def X():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.demod")


@pytest.fixture(scope="module")
def K():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")


# ------------------------------------------------------------------------------------------ header, exports, binding
def test_header_is_c99_and_matches_the_exports_and_the_binding(X, tmp_path):
    text, _ = check_header_exports_binding(BY_MODULE["demod"], X, tmp_path, "typedef kdm_demod* handle;\n",
                                           ["KDM_MAX_TAPS", "KDM_MODE_PM", "KDM_OUT_S16"])
    for name, value in (("KDM_MAX_DECIM", X.MAX_DECIM), ("KDM_MAX_TAPS", X.MAX_TAPS), ("KDM_MAX_IN", X.MAX_IN),
                        ("KDM_MODE_AM", X.MODE_AM), ("KDM_MODE_FM", X.MODE_FM), ("KDM_MODE_PM", X.MODE_PM),
                        ("KDM_OUT_F32", X.OUT_F32), ("KDM_OUT_S16", X.OUT_S16)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value, name
    assert (X.MODE_AM, X.MODE_FM, X.MODE_PM, X.OUT_F32, X.OUT_S16) == (mm.MODE_AM, mm.MODE_FM, mm.MODE_PM, mm.OUT_F32, mm.OUT_S16)


def test_the_other_bindings_hold_no_kdm_name_and_the_package_exports_the_class(X):
    others = [importlib.import_module("prgs-sdr-kspecanal_amd." + m) for m in ("_lib", "density", "mask", "ddc", "detect")]
    assert not [n for m in others for n in m.SIGNATURES if n.startswith("kdm_")]
    assert all(n.startswith("kdm_") for n in X.SIGNATURES)
    pkg = load_pkg()
    for name in ("Demodulator", "demod_taps", "write_wav"):
        assert getattr(pkg, name) is getattr(X, name) and name in pkg.__all__
    for name in ("process_dev", "process", "out_count", "blocks_dev", "block_out_count", "read_out", "set_taps", "reset", "state",
                 "kernel_info", "set_stream", "synchronize", "close"):
        assert callable(getattr(X.Demodulator, name)), name
    assert isinstance(X.Demodulator.out, property)


def test_library_loads_without_a_gpu_and_there_is_no_fallback(X):
    lib = X.load()
    assert lib.kdm_abi_version() == X.ABI_VERSION
    try:
        import torch
        have_gpu = torch.cuda.is_available()
    except ImportError:
        have_gpu = False
    if not have_gpu:
        with pytest.raises(X.KsaError):
            X.Demodulator("fm", 4, np.ones(8, dtype=np.float32))
    with pytest.raises(X.KsaError, match="__graft_entry__"):
        X.load(os.path.join(PKG_DIR, "no_such_libksa_demod.so"))
    with pytest.raises(X.KsaError, match=r"unknown mode \[ssb\]"):              # the binding's own refusals come before the library
        X.Demodulator("ssb", 4, np.ones(8, dtype=np.float32))
    with pytest.raises(X.KsaError, match=r"unknown out_fmt \[u8\]"):
        X.Demodulator("fm", 4, np.ones(8, dtype=np.float32), out_fmt="u8")
    # create-time refusals need no device: each has its own text and leaves a null handle
    taps = np.ones(8, dtype=np.float32)
    nan, inf = taps.copy(), taps.copy()
    nan[3], inf[5] = np.nan, np.inf
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    texts = []
    # (device, mode, decim, ntaps, taps, out_fmt, pcm_scale, max_in)
    for args, text in (((0, 3, 4, 8, p(taps), 0, 1.0, 64), "unknown mode 3"), ((0, -1, 4, 8, p(taps), 0, 1.0, 64), "unknown mode -1"),
                       ((0, 1, 4, 8, p(taps), 2, 1.0, 64), "unknown output format 2"), ((0, 1, 4, 8, p(taps), -1, 1.0, 64), "unknown output format -1"),
                       ((0, 1, 0, 8, p(taps), 0, 1.0, 64), "decim 0"), ((0, 1, 257, 8, p(taps), 0, 1.0, 64), "decim 257"),
                       ((0, 1, 4, 0, p(taps), 0, 1.0, 64), "ntaps 0"), ((0, 1, 4, 4097, p(taps), 0, 1.0, 64), "ntaps 4097"),
                       ((0, 1, 4, 8, p(taps), 0, 1.0, 0), "max_in 0"), ((0, 1, 4, 8, p(taps), 0, 1.0, 2 ** 28), "max_in 268435456"),
                       ((0, 1, 4, 8, None, 0, 1.0, 64), "null taps"), ((0, 1, 4, 8, p(nan), 0, 1.0, 64), "tap 3 is not finite"),
                       ((0, 1, 4, 8, p(inf), 0, 1.0, 64), "tap 5 is not finite"),
                       ((0, 1, 4, 8, p(taps), 1, 0.0, 64), "pcm_scale 0"), ((0, 1, 4, 8, p(taps), 1, -2.0, 64), "pcm_scale -2"),
                       ((0, 1, 4, 8, p(taps), 1, np.inf, 64), "pcm_scale inf"), ((0, 1, 4, 8, p(taps), 1, np.nan, 64), "pcm_scale nan"),
                       ((-1, 1, 4, 8, p(taps), 0, 1.0, 64), "device -1")):
        h = C.c_void_p(1)
        assert lib.kdm_create(*args, C.byref(h)) != 0 and h.value is None, text
        got = lib.kdm_last_error().decode()
        assert text in got, (text, got)
        texts.append(re.sub(r"-?(inf|nan|[0-9][0-9.e+]*)", "#", got))
    assert len(set(texts)) == 9, sorted(set(texts))     # mode / format / decim / ntaps / max_in / null taps / tap / pcm_scale / device
    # pcm_scale is only read for int16 output; only a device is missing then
    if not have_gpu:
        h = C.c_void_p(1)
        assert lib.kdm_create(0, 1, 4, 8, p(taps), 0, 0.0, 64, C.byref(h)) != 0 and h.value is None
        assert "hip" in lib.kdm_last_error().decode()
    # a null object is refused by every entry point that takes one
    n = C.c_int64()
    for call in (lambda: lib.kdm_out_count(None, 1, C.byref(n)), lambda: lib.kdm_process_dev(None, None, 0, None, 0, None),
                 lambda: lib.kdm_process(None, None, 0, None, 0, None), lambda: lib.kdm_blocks_dev(None, None, 0, 0, 0, None, 0),
                 lambda: lib.kdm_set_taps(None, None), lambda: lib.kdm_reset(None), lambda: lib.kdm_state(None, None, None),
                 lambda: lib.kdm_out_dev(None, None, None), lambda: lib.kdm_read_out(None, None, 0, 0),
                 lambda: lib.kdm_kernel_info(None, None, None, None, None, None), lambda: lib.kdm_set_stream(None, None),
                 lambda: lib.kdm_synchronize(None)):
        assert call() != 0 and "null demodulator" in lib.kdm_last_error().decode()
    lib.kdm_destroy(None)
    assert len(X.SIGNATURES) == 12 + 4                  # the twelve above, abi_version, last_error, create, destroy


# ------------------------------------------------------------------------------------------ the model checks itself
def test_model_axis_rule_and_detector():
    neg0 = -0.0
    assert np.array_equal(mm.turns([0, neg0, 2, 2, -2, -2, 0, neg0, 0, neg0], [0, neg0, 0, neg0, 0, neg0, 3, 3, -3, -3]),
                          [0, 0, 0, 0, 0.5, 0.5, 0.25, 0.25, -0.25, -0.25])
    assert np.arctan2(neg0, -2.0) < 0                    # what np.arctan2 alone would give: -0.5 turn
    assert np.array_equal(mm.f32_turns([0, neg0, 2, 2, -2, -2, 0, neg0, 0, neg0], [0, neg0, 0, neg0, 0, neg0, 3, 3, -3, -3]),
                          np.array([0, 0, 0, 0, 0.5, 0.5, 0.25, 0.25, -0.25, -0.25], dtype=np.float32))
    x = np.array([1, 1j, -1, -1j, 1 + 1j, 0], dtype=np.complex128)
    assert np.allclose(mm.detect(x, mm.MODE_AM), [1, 1, 1, 1, np.sqrt(2), 0], rtol=0, atol=1e-15)
    assert np.allclose(mm.detect(x, mm.MODE_PM), [0, 0.25, 0.5, -0.25, 0.125, 0], rtol=0, atol=1e-15)
    assert np.allclose(mm.detect(x, mm.MODE_FM), [0, 0.25, 0.25, 0.25, 0.375, 0], rtol=0, atol=1e-15)
    tone = np.exp(2j * np.pi * 0.05 * np.arange(50))
    assert np.allclose(mm.detect(tone, mm.MODE_FM)[1:], 0.05, rtol=0, atol=1e-12)       # cycles per sample


def _lfilter(h, v):
    y = np.zeros(len(v))
    for n in range(len(v)):
        for k in range(len(h)):
            if n - k >= 0:
                y[n] += h[k] * v[n - k]
    return y


def test_model_stream_is_a_filter_followed_by_decimation():
    rng = np.random.default_rng(5)
    for mode in MODES:
        for D, T, n in ((1, 1, 7), (3, 5, 40), (4, 9, 41), (7, 3, 50)):
            x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
            h = rng.standard_normal(T)
            want = _lfilter(h, mm.detect(x, mode))[::D]
            got = mm.stream(x, h, D, mode)
            assert got.shape == want.shape == (-(-n // D),) and np.allclose(got, want, rtol=0, atol=1e-12)
            assert np.allclose(mm.fir_at(mm.detect(x, mode), h, D, 0, len(want)), want, rtol=0, atol=1e-12)
        assert mm.stream(np.zeros(0), [1.0], 2, mode).shape == (0,)


def test_model_block_form_is_the_stream_form_past_its_transient():
    rng = np.random.default_rng(6)
    for mode in MODES:
        ld = mm.lead(mode)
        for D, T, M in ((1, 4, 9), (3, 7, 5), (4, 9, 6), (5, 1, 4)):
            L = ld + D * (M - 1) + T + (D - 1)               # up to D - 1 further samples: no further output
            assert mm.block_out_count(L, T, D, mode) == M
            x = rng.standard_normal((2, L)) + 1j * rng.standard_normal((2, L))
            h = rng.standard_normal(T)
            b = mm.blocks(x, h, D, mode)
            assert b.shape == (2, M)
            for row, got in zip(x, b):
                # block output m is the undecimated filter's output at lead + T-1 + m D
                full = _lfilter(h, mm.detect(row, mode))
                assert np.allclose(got, full[ld + T - 1::D][:M], rtol=0, atol=1e-12)
                assert np.allclose(mm.fir_at(mm.detect(row, mode), h, D, ld + T - 1, M), got, rtol=0, atol=1e-12)


def test_model_out_count_over_random_cuts():
    rng = np.random.default_rng(7)
    for D in (1, 2, 3, 16, 256):
        at, total = 0, 0
        for c in rng.integers(0, 3 * D + 2, 200):
            k = mm.out_count(at, int(c), D)
            assert k == len(range(-(-at // D) * D, at + int(c), D))          # the multiples of D in [at, at + c)
            at, total = at + int(c), total + k
        assert total == -(-at // D)


def test_exact_model_matches_the_float_model_on_exact_inputs():
    rng = np.random.default_rng(8)
    n, D = 60, 3
    for taps in (rng.integers(-8, 9, 11).astype(np.float64), np.array([0.5, -0.25, 2.0, 1.0, 0.125])):
        T = len(taps)
        for mode in MODES:
            if mode == mm.MODE_AM:
                x, mag = mm.exact_am_samples(rng, n)
                dn, dden = mm.exact_detect(mode, mag=mag)
                k = None
            else:
                x, k = mm.exact_turn_samples(rng, n)
                dn, dden = mm.exact_detect(mode, k=k)
            assert np.array_equal(dn / dden, mm.detect(x, mode))
            assert np.array_equal(mm.f32_detect(x, mode), (dn / dden).astype(np.float32))        # the float32 steps are exact too
            want = mm.stream(x, taps, D, mode)
            assert np.allclose(mm.exact_stream(dn, dden, taps, D), want, rtol=0, atol=1e-9)
            assert np.array_equal(mm.exact_stream(dn, dden, taps, D, mm.OUT_S16, 64.0), mm.pcm(want, 64.0))
            L, starts = T + 20, [0, 7, 25]
            wb = mm.blocks(np.array([x[s:s + L] for s in starts]), taps, D, mode)
            assert np.allclose(mm.exact_blocks(dn, dden, taps, D, mode, starts, L), wb, rtol=0, atol=1e-9)
            for backwards in (False, True):
                assert np.array_equal(mm.f32_fir(mm.f32_detect(x, mode), taps, D, 0, len(want), backwards),
                                      mm.exact_stream(dn, dden, taps, D))
    # the int16 rule in integers: half to even, saturation at both ends
    num = np.array([1, 3, -1, -3, 5, 70000, -70000], dtype=np.int64)
    assert np.array_equal(mm._exact_out(num, 2, mm.OUT_S16, 1.0), [0, 2, 0, -2, 2, 32767, -32768])


@pytest.mark.parametrize("shape", EMU_SHAPES, ids=str)
def test_float32_emulation_leaves_the_bound_ample_room(shape):
    """The premise of the GPU float test: a sequential float32 emulation (the detector's float32 steps and one fused
    multiply-add per tap) stays at or below 6 % of the bound sum|h| ((T + 16) 2^-24 dmax + B), and the detector alone within half
    of B's units (8 for FM and PM, 4 for AM; the emulation peaks at 0.99 of one unit)."""
    D, T = shape
    t = np.arange(T, dtype=np.float64) - (T - 1) / 2
    taps = np.sinc(0.8 * t / D) * np.hamming(T)
    taps = (taps / taps.sum()).astype(np.float32)
    count = 300 if T < 1024 else 40
    n = D * (count - 1) + 1
    for mode in MODES:
        rng = np.random.default_rng(D * 31337 + T + mode)
        x = mm.float_input(rng, n, mode)
        d64, d32 = mm.detect(x, mode), mm.f32_detect(x, mode)
        scale = np.abs(x).max() if mode == mm.MODE_AM else 1.0
        units = np.max(np.abs(d32 - d64)) / (mm.UNIT * scale)
        want = mm.fir_at(d64, taps, D, 0, count)
        emu = mm.f32_fir(d32, taps, D, 0, count)
        ratio = np.max(np.abs(emu - want)) / mm.bound(taps, mode, np.abs(x).max())
        print("demod emulation %s mode %d: detector %.3f units, error / bound %.4f" % (shape, mode, units, ratio))
        assert units <= (2.0 if mode == mm.MODE_AM else 4.0) and ratio <= 0.06, (shape, mode, units, ratio)


# ------------------------------------------------------------------------------------------ the helpers
def _response(h, f):
    return abs(np.sum(h.astype(np.float64) * np.exp(-2j * np.pi * f * np.arange(len(h)))))


def test_demod_taps_gain_deemphasis_and_dc_block(X):
    ddc = importlib.import_module("prgs-sdr-kspecanal_amd.ddc")
    for D, tpp, gain in ((1, 1, 1.0), (5, 8, 1.0), (5, 32, 4.0), (16, 8, 0.25), (256, 16, 1.0)):
        h = X.demod_taps(D, tpp, gain=gain)
        assert h.dtype == np.float32 and h.shape == (D * tpp,) and abs(float(h.astype(np.float64).sum()) - gain) <= 1e-6 * gain + 1e-6
        assert np.allclose(h, gain * ddc.ddc_lowpass(D, tpp), rtol=0, atol=1e-6 * gain)
    fs, tau = 240e3, 75e-6
    plain, de = X.demod_taps(5, 32), X.demod_taps(5, 32, deemph_us=75, sampling_rate=fs)
    assert de.shape == plain.shape and abs(float(de.astype(np.float64).sum()) - 1) <= 1e-6
    corner = 1 / (2 * np.pi * tau) / fs
    drop = 20 * np.log10(_response(de, corner) / _response(plain, corner))
    assert abs(drop + 3.0) <= 0.2, drop
    for D, tpp in ((1, 8), (5, 8), (16, 8)):
        h = X.demod_taps(D, tpp, dc_block=True).astype(np.float64)
        assert abs(h.sum()) <= 1e-6 * np.abs(h).sum()
    for bad in (lambda: X.demod_taps(0), lambda: X.demod_taps(257), lambda: X.demod_taps(256, 17), lambda: X.demod_taps(4, 8, 0.0),
                lambda: X.demod_taps(4, 8, deemph_us=75), lambda: X.demod_taps(4, 8, deemph_us=0, sampling_rate=48e3)):
        with pytest.raises(X.KsaError):
            bad()


def test_write_wav_round_trips(X, tmp_path):
    pcm = np.array([0, 1, -1, 32767, -32768, 1234, -4321], dtype=np.int16)
    path = tmp_path / "a.wav"
    X.write_wav(path, pcm, 48000)
    with wave.open(str(path), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 48000, len(pcm))
        assert np.array_equal(np.frombuffer(w.readframes(len(pcm)), dtype="<i2"), pcm)
    with pytest.raises(X.KsaError):
        X.write_wav(path, pcm.astype(np.float32), 48000)


# ------------------------------------------------------------------------------------------ command line
def test_demod_key_parses_in_each_form(K, capsys):
    base = ["zeroSpan", "fftSize", "1024", "zoom", "10:300e3", "demod"]
    d = K.handle_args({}, base + ["fm"])
    full, fs = d["fullSize"], d["samplingRate"]
    assert d["demod.spec"] == dict(mode="fm", decim=1, taps_per_phase=8, ntaps=8, deemph_us=None, out_per_block=full - 1 - 8 + 1,
                                   rate=int(fs / 10))
    s = K.handle_args({}, base + ["FM:5"])["demod.spec"]
    assert (s["mode"], s["decim"], s["ntaps"], s["out_per_block"], s["rate"]) == ("fm", 5, 40, (full - 1 - 40) // 5 + 1, 48000)
    s = K.handle_args({}, base + ["am:4:16"])["demod.spec"]
    assert (s["mode"], s["decim"], s["taps_per_phase"], s["ntaps"], s["out_per_block"], s["rate"]) == ("am", 4, 16, 64, (full - 64) // 4 + 1, 60000)
    s = K.handle_args({}, base + ["pm:5:8:75"])["demod.spec"]
    assert (s["mode"], s["deemph_us"], s["out_per_block"]) == ("pm", 75.0, (full - 40) // 5 + 1)
    capsys.readouterr()
    s = K.handle_args({}, ["zeroSpan", "fftSize", "1024", "zoom", "1", "demod", "fm:7", "demodSave", "x.wav"])     # zoom 1: the whole band
    assert s["demod.spec"]["rate"] == round(fs / 7) and s["demodSave"] == "x.wav" and "WARN" in capsys.readouterr().out
    d = K.handle_args({}, ["zeroSpan", "fftSize", "1024", "iqFormat", "s16", "frameBatch", "4", "zoom", "4:1e5:2", "demod", "am:2", "density",
                           "64:-120:0", "mask", "flat:-50", "detect", "8:2:10"])              # it combines with the other keys
    assert d["demod.spec"] and d["zoom.spec"] and d["density.spec"] and d["mask.spec"] and d["detect.spec"]
    d = K.handle_args({}, ["zeroSpan", "fftSize", "1024"])
    assert d["demod"] == "" and d["demodSave"] == "" and d["demod.spec"] is None
    capsys.readouterr()
    K.handle_args({}, ["zeroSpan", "fftSize", "1024", "demodSave", "x.wav"])
    assert "WARN" in capsys.readouterr().out


@pytest.mark.parametrize("value", ["x", "ssb", "fm:", "fm:0", "fm:257", "fm:-4", "fm:2.5", "fm:x", "fm:5:0", "fm:5:x", "fm:256:17", "fm:5:8:0",
                                   "fm:5:8:-75", "fm:5:8:nan", "fm:5:8:inf", "fm:5:8:x", "fm:5:8:75:1", ":", "fm:5:8:", "am:256:16"])
def test_demod_key_refuses_with_the_rule(K, value, capsys):
    d = {}
    with pytest.raises(SystemExit):
        K.handle_args(d, ["zeroSpan", "fftSize", "64", "samplingRate", "256", "zoom", "1", "demod", value])
    assert d["cmd.stop"] is True
    assert K.DEMOD_RULE in capsys.readouterr().out


def test_demod_is_zerospan_only_and_needs_zoom(K, capsys):
    for mode in (["scan", "startFreq", "100e6", "endFreq", "104.8e6"], ["fmScan"], ["quickFullScan"], ["zeroSpanSave"]):
        with pytest.raises(SystemExit):
            K.handle_args({}, mode + ["demod", "fm"])
        assert "zeroSpan only" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        K.handle_args({}, ["zeroSpan", "bUsePSD", "true", "demod", "fm"])
    assert "bUsePSD false" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        K.handle_args({}, ["zeroSpan", "fftSize", "1024", "demod", "fm"])                      # no zoom
    assert K.DEMOD_RULE in capsys.readouterr().out
    d = K.handle_args({}, ["zeroSpanPlay", "fftSize", "512", "zoom", "16", "demod", "fm"])
    assert d["demod.spec"] is None and "WARN" in capsys.readouterr().out


def test_defaults_leave_the_reference_cases_alone(K):
    cli = json.load(open(os.path.join(GOLDEN, "cli_args.json")))
    for name, case in cli.items():
        d = K.handle_args({}, case["argv"] + ["prgLoopCnt", "0"])
        for k, want in case["d"].items():
            assert d[k] == want, (name, k)
        assert d["demod.spec"] is None and d["demod"] == "" and d["demodSave"] == ""


# ------------------------------------------------------------------------------------------ resources
def test_every_demod_kernel_runs_without_scratch(tmp_path):
    kernels = _kernels(_asm(os.path.join(PKG_DIR, "csrc_demod", "kdm_api.hip"), str(tmp_path / "kdm_api.s")))
    names = sorted(kernels)
    assert len([k for k in names if "tile_kernel<" in k]) == 12, names          # 3 modes x 4, 1 outputs per thread x 2 output formats
    assert len([k for k in names if "history_kernel<" in k]) == 3, names
    assert len(names) == 15
    for k in names:
        assert _resource(kernels[k][1], "ScratchSize") == 0, k
