"""Host side of the digital down-converter (no GPU needed): the companion header and library, the binding, the models every GPU
test compares against, the helpers, the `zoom` key of the command line, and the kernels' resource report."""
import ctypes as C
import importlib
import json
import os
import re

import numpy as np
import pytest

import ddc_model as dm
from companion_helper import BY_MODULE, check_header_exports_binding
from conftest import GOLDEN, ROOT, load_pkg
from test_isa_regression import _asm, _kernels, _resource

PKG_DIR = os.path.join(ROOT, "prgs-sdr-kspecanal_amd")
SHAPES = [(1, 1), (1, 33), (2, 16), (3, 11), (4, 32), (5, 35), (16, 128), (64, 1024), (1024, 16384)]
INC = round(0.1234567 * 2 ** 64)


@pytest.fixture(scope="module")
def X():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.ddc")


@pytest.fixture(scope="module")
def K():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")


# ------------------------------------------------------------------------------------------ header, exports, binding
def test_header_is_c99_and_matches_the_exports_and_the_binding(X, tmp_path):
    text, _ = check_header_exports_binding(BY_MODULE["ddc"], X, tmp_path, "typedef kdc_ddc* handle;\n",
                                           ["KDC_MAX_TAPS", "KDC_FMT_S16", "KDC_FORM_REDUCE"])
    for name, value in (("KDC_MAX_DECIM", X.MAX_DECIM), ("KDC_MAX_TAPS", X.MAX_TAPS), ("KDC_MAX_IN", X.MAX_IN),
                        ("KDC_FORM_TILE", X.FORM_TILE), ("KDC_FORM_REDUCE", X.FORM_REDUCE)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value, name
    pkg = load_pkg()
    assert [int(re.search(r"#define KDC_FMT_%s (\d+)" % n, text).group(1)) for n in ("C64", "U8", "S8", "S16")] == \
        [pkg.FMT_C64, pkg.FMT_U8, pkg.FMT_S8, pkg.FMT_S16] == [dm.FMT_C64, dm.FMT_U8, dm.FMT_S8, dm.FMT_S16]


def test_the_other_bindings_hold_no_kdc_name_and_the_package_exports_the_class(X):
    lib = importlib.import_module("prgs-sdr-kspecanal_amd._lib")
    dens = importlib.import_module("prgs-sdr-kspecanal_amd.density")
    mask = importlib.import_module("prgs-sdr-kspecanal_amd.mask")
    assert not [n for n in list(lib.SIGNATURES) + list(dens.SIGNATURES) + list(mask.SIGNATURES) if n.startswith("kdc_")]
    assert all(n.startswith("kdc_") for n in X.SIGNATURES)
    pkg = load_pkg()
    for name in ("DownConverter", "ddc_lowpass", "phase_inc_for"):
        assert getattr(pkg, name) is getattr(X, name) and name in pkg.__all__
    for name in ("process_dev", "process", "blocks_dev", "out_count", "retune", "set_taps", "reset", "state", "kernel_info", "close"):
        assert callable(getattr(X.DownConverter, name)), name
    assert isinstance(X.DownConverter.out, property)


def test_library_loads_without_a_gpu_and_there_is_no_fallback(X):
    lib = X.load()
    assert lib.kdc_abi_version() == X.ABI_VERSION
    try:
        import torch
        have_gpu = torch.cuda.is_available()
    except ImportError:
        have_gpu = False
    if not have_gpu:
        with pytest.raises(X.KsaError):
            X.DownConverter(dm.FMT_C64, 4, np.ones(8, dtype=np.float32))
    with pytest.raises(X.KsaError, match="__graft_entry__"):
        X.load(os.path.join(PKG_DIR, "no_such_libksa_ddc.so"))
    # create-time refusals need no device: each has its own text and leaves a null handle
    taps = np.ones(8, dtype=np.float32)
    nan, inf = taps.copy(), taps.copy()
    nan[3], inf[5] = np.nan, np.inf
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    texts = []
    # (device, fmt, u8_offset, u8_scale, decim, ntaps, taps, phase_inc, max_in)
    for args, text in (((0, 0, 0.0, 1.0, 0, 8, p(taps), 0, 64), "decim 0"), ((0, 0, 0.0, 1.0, 1025, 8, p(taps), 0, 64), "decim 1025"),
                       ((0, 0, 0.0, 1.0, 4, 0, p(taps), 0, 64), "ntaps 0"), ((0, 0, 0.0, 1.0, 4, 16385, p(taps), 0, 64), "ntaps 16385"),
                       ((0, 0, 0.0, 1.0, 4, 8, p(taps), 0, 0), "max_in 0"), ((0, 0, 0.0, 1.0, 4, 8, p(taps), 0, 2 ** 28), "max_in 268435456"),
                       ((0, 0, 0.0, 1.0, 4, 8, None, 0, 64), "null taps"), ((0, 0, 0.0, 1.0, 4, 8, p(nan), 0, 64), "tap 3 is not finite"),
                       ((0, 0, 0.0, 1.0, 4, 8, p(inf), 0, 64), "tap 5 is not finite"),
                       ((0, 4, 0.0, 1.0, 4, 8, p(taps), 0, 64), "unknown sample format 4"), ((0, -1, 0.0, 1.0, 4, 8, p(taps), 0, 64), "unknown sample format -1"),
                       ((0, 1, 0.0, 0.0, 4, 8, p(taps), 0, 64), "u8_scale 0"), ((0, 1, 0.0, np.inf, 4, 8, p(taps), 0, 64), "u8_scale inf"),
                       ((0, 1, np.nan, 1.0, 4, 8, p(taps), 0, 64), "u8_offset nan"), ((-1, 0, 0.0, 1.0, 4, 8, p(taps), 0, 64), "device -1")):
        h = C.c_void_p(1)
        assert lib.kdc_create(*args, C.byref(h)) != 0 and h.value is None, text
        got = lib.kdc_last_error().decode()
        assert text in got, (text, got)
        texts.append(re.sub(r"-?(inf|nan|[0-9][0-9.e+]*)", "#", got))
    assert len(set(texts)) == 9, sorted(set(texts))     # decim / ntaps / max_in / null taps / tap / format / u8_scale / u8_offset / device
    # a zero u8_scale is only read for uint8 input; only a device is missing then
    if not have_gpu:
        h = C.c_void_p(1)
        assert lib.kdc_create(0, 0, 0.0, 0.0, 4, 8, p(taps), 0, 64, C.byref(h)) != 0 and h.value is None
        assert "hip" in lib.kdc_last_error().decode()
    # a null object is refused by every entry point that takes one
    n = C.c_int64()
    for call in (lambda: lib.kdc_out_count(None, 1, C.byref(n)), lambda: lib.kdc_process_dev(None, None, 0, None, 0, None),
                 lambda: lib.kdc_process(None, None, 0, None, 0, None), lambda: lib.kdc_blocks_dev(None, None, 0, 0, 0, None, 0),
                 lambda: lib.kdc_set_tuning(None, 0), lambda: lib.kdc_set_taps(None, None), lambda: lib.kdc_reset(None),
                 lambda: lib.kdc_state(None, None, None, None), lambda: lib.kdc_out_dev(None, None, None),
                 lambda: lib.kdc_kernel_info(None, None, None, None, None, None, None), lambda: lib.kdc_set_stream(None, None),
                 lambda: lib.kdc_synchronize(None)):
        assert call() != 0 and "null down-converter" in lib.kdc_last_error().decode()
    lib.kdc_destroy(None)


# ------------------------------------------------------------------------------------------ the model checks itself
def _lfilter(h, v):
    y = np.zeros(len(v), dtype=np.complex128)
    for n in range(len(v)):
        for k in range(len(h)):
            if n - k >= 0:
                y[n] += h[k] * v[n - k]
    return y


def test_model_stream_is_a_filter_followed_by_decimation():
    rng = np.random.default_rng(5)
    for D, T, n in ((1, 1, 7), (3, 5, 40), (4, 9, 41), (7, 3, 50)):
        x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        h = rng.standard_normal(T)
        phi = dm.phases(n, INC)
        v = x * np.exp(-2j * np.pi * np.array([(i * INC % 2 ** 64) / 2 ** 64 for i in range(n)]))
        want = _lfilter(h, v)[::D]
        got = dm.stream(x, h, D, phi)
        assert got.shape == want.shape == (-(-n // D),) and np.allclose(got, want, rtol=0, atol=1e-12)
        assert np.allclose(dm.fir_at(x * dm.rotor(phi), h, D, 0, len(want)), want, rtol=0, atol=1e-12)
    assert dm.stream(np.zeros(0), [1.0], 2, dm.phases(0, INC)).shape == (0,)


def test_model_block_form_is_the_stream_form_past_its_transient():
    rng = np.random.default_rng(6)
    for D, T, M in ((1, 4, 9), (3, 7, 5), (4, 9, 6), (5, 1, 4)):            # (T - 1) % D == 0: block output m is stream output m + (T-1)/D
        assert (T - 1) % D == 0
        L = D * (M - 1) + T
        x = rng.standard_normal((2, L)) + 1j * rng.standard_normal((2, L))
        h = rng.standard_normal(T)
        b = dm.blocks(x, h, D, INC)
        assert b.shape == (2, M)
        for row, got in zip(x, b):
            s = dm.stream(row, h, D, dm.phases(L, INC))
            assert np.allclose(got, s[(T - 1) // D:], rtol=0, atol=1e-12) and len(s) == M + (T - 1) // D
            assert np.allclose(dm.fir_at(row * dm.rotor(dm.phases(L, INC)), h, D, T - 1, M), got, rtol=0, atol=1e-12)
    extra = dm.blocks(rng.standard_normal((1, 3 * 4 + 9 + 3)), np.ones(9), 4, 0)     # up to D - 1 further samples: no further output
    assert extra.shape == (1, 4)


def test_model_out_count_over_random_cuts():
    rng = np.random.default_rng(7)
    for D in (1, 2, 3, 16, 1024):
        at, total = 0, 0
        for c in rng.integers(0, 3 * D + 2, 200):
            k = dm.out_count(at, int(c), D)
            assert k == len(range(-(-at // D) * D, at + int(c), D))          # the multiples of D in [at, at + c)
            at, total = at + int(c), total + k
        assert total == -(-at // D)


def test_integer_model_matches_the_float_model_at_quarter_turns():
    rng = np.random.default_rng(8)
    n, D, taps = 50, 3, rng.integers(-8, 9, 11)
    for fmt, raw in ((dm.FMT_S16, rng.integers(-32768, 32768, 2 * n).astype(np.int16)), (dm.FMT_S8, rng.integers(-128, 128, 2 * n).astype(np.int8)),
                     (dm.FMT_U8, rng.integers(0, 256, 2 * n).astype(np.uint8)),
                     (dm.FMT_C64, ((rng.integers(-999, 999, n) + 1j * rng.integers(-999, 999, n)) / 32768).astype(np.complex64))):
        kw = dict(u8_offset=128.0, u8_scale=128.0)
        iq, scale = dm.to_int(raw, fmt)
        for inc in (0, 2 ** 62, 2 ** 63, 3 * 2 ** 62):
            phi = dm.phases(n, inc)
            want = dm.stream(dm.unpack(raw, fmt, **kw), taps, D, phi)
            assert np.allclose(dm.int_stream(iq, scale, taps, D, phi), want, rtol=0, atol=1e-6), (fmt, inc)
            assert np.array_equal(dm.f32_mix(dm.unpack(raw, fmt, **kw).astype(np.complex64), phi),
                                  (dm.unpack(raw, fmt, **kw) * np.round(dm.rotor(phi))).astype(np.complex64))     # exact at quarter turns
            wb = dm.blocks(dm.unpack(raw, fmt, **kw)[None, :], taps, D, inc)
            assert np.allclose(dm.int_blocks(iq, scale, taps, D, inc, 1, n, [0]), wb, rtol=0, atol=1e-6)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_float32_emulation_leaves_the_bound_ample_room(shape):
    """The premise of the GPU float test: a sequential float32 emulation (the mixer's steps and one fused multiply-add per tap)
    stays below 6 % of the bound (T + 16) 2^-24 sum|h| max|x|.  At T = 1 the sum contributes nothing and what is left is the
    mixer alone, which the bound's own budget puts at angle 1.6 + sin / cos 2 + product 3 = 6.6 of its 17 units; the
    emulation measures about 1.6 units there (9 %), so that shape is held to the budget, not to 6 %."""
    D, T = shape
    t = np.arange(T, dtype=np.float64) - (T - 1) / 2
    taps = np.sinc(0.8 * t / D) * np.hamming(T)
    taps = (taps / taps.sum()).astype(np.float32)
    count = 3 * (8 if D == 1024 else 256) + 7
    n = D * (count - 1) + 1
    rng = np.random.default_rng(D * 31337 + T)
    x = (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)
    phi = dm.phases(n, INC)
    want = dm.fir_at(x.astype(np.complex128) * dm.rotor(phi), taps, D, 0, count)
    emu = dm.f32_fir(dm.f32_mix(x, phi), taps, D, 0, count)
    ratio = np.max(np.abs(emu - want)) / dm.bound(taps, np.abs(x).max())
    assert ratio <= (6.6 / 17 if T == 1 else 0.06), ratio


# ------------------------------------------------------------------------------------------ the helpers
def test_phase_inc_for_is_exact(X):
    assert X.phase_inc_for(1, 4) == 2 ** 62 and X.phase_inc_for(600e3, 2.4e6) == 2 ** 62
    assert X.phase_inc_for(1, 3) == (2 ** 64 + 1) // 3 == 6148914691236517205      # float64 * 2^64 would end in zeros
    assert X.phase_inc_for(-1, 4) == 3 * 2 ** 62 and X.phase_inc_for(0, 1) == 0 and X.phase_inc_for(5, 4) == 2 ** 62
    assert X.phase_inc_for(1, 2 ** 64) == 1 and X.phase_inc_for(-1, 2 ** 64) == 2 ** 64 - 1


def test_ddc_lowpass_sums_to_one_and_cuts_where_it_says(X):
    for D, tpp, cutoff, window in ((1, 1, 0.8, "hamming"), (4, 8, 0.8, "hamming"), (16, 8, 0.8, "hamming"), (16, 16, 0.5, "hanning"),
                                   (64, 8, 1.0, "hamming"), (5, 7, 0.8, "hamming")):
        h = X.ddc_lowpass(D, tpp, cutoff, window)
        assert h.dtype == np.float32 and h.shape == (D * tpp,) and abs(float(h.astype(np.float64).sum()) - 1) < 1e-6
        assert np.allclose(h, h[::-1], rtol=0, atol=1e-9)
        if tpp < 4:
            continue
        grid = 4096                                      # the frequency grid, fs / 4096: 8 and more points per lobe fs / T of these filters
        H = np.abs(np.fft.rfft(h.astype(np.float64), grid))
        first_below = int(np.argmax(H < 0.5))            # the -6 dB point, in grid steps
        assert abs(first_below - cutoff * grid / (2 * D)) <= 1, (D, tpp, cutoff, first_below)
    for bad in (lambda: X.ddc_lowpass(0), lambda: X.ddc_lowpass(1025), lambda: X.ddc_lowpass(1024, 17), lambda: X.ddc_lowpass(4, 8, 0.0)):
        with pytest.raises(X.KsaError):
            bad()


# ------------------------------------------------------------------------------------------ command line
def test_zoom_key_parses_in_each_form(K):
    base = ["zeroSpan", "fftSize", "1024", "zoom"]
    d = K.handle_args({}, base + ["16"])
    full, fs, fc = d["fullSize"], d["samplingRate"], d["centerFreq"]
    assert d["zoom.spec"] == dict(decim=16, offset=0.0, taps_per_phase=8, ntaps=128, block_len=16 * (full - 1) + 128, center=fc, span=fs / 16)
    assert (d["startFreq"], d["endFreq"]) == (fc - fs / 32, fc + fs / 32)
    s = K.handle_args({}, base + ["16:300e3"])["zoom.spec"]
    assert (s["decim"], s["offset"], s["taps_per_phase"], s["center"]) == (16, 300e3, 8, fc + 300e3)
    s = K.handle_args({}, base + ["1024:-1.2e6:16"])["zoom.spec"]
    assert (s["decim"], s["offset"], s["ntaps"], s["block_len"]) == (1024, -1.2e6, 16384, 1024 * (full - 1) + 16384)
    s = K.handle_args({}, base + ["1::"[:1]])["zoom.spec"]
    assert (s["decim"], s["ntaps"], s["block_len"], s["span"]) == (1, 8, full - 1 + 8, fs)
    d = K.handle_args({}, ["zeroSpan", "fftSize", "1024", "iqFormat", "s16", "frameBatch", "4", "zoom", "4:1e5:2", "density", "64:-120:0",
                           "mask", "flat:-50", "pfbTaps", "4"])                       # it combines with the other keys
    assert d["zoom.spec"]["block_len"] == 4 * (4 * 1024 - 1) + 8 and d["density.spec"] and d["mask.spec"]
    d = K.handle_args({}, ["zeroSpan", "fftSize", "1024"])
    assert d["zoom"] == "" and d["zoom.spec"] is None


@pytest.mark.parametrize("value", ["x", "0", "1025", "-4", "2.5", "16:", "16:x", "16:nan", "16:inf", "16:1.3e6", "16:-1.3e6", "16:0:0", "16:0:17",
                                   "16:0:x", "16:0:8:1", "1024:0:16:", ":", "16:0:2.5"])
def test_zoom_key_refuses_with_the_rule(K, value, capsys):
    d = {}
    with pytest.raises(SystemExit):
        K.handle_args(d, ["zeroSpan", "fftSize", "1024", "zoom", value])
    assert d["cmd.stop"] is True
    assert K.ZOOM_RULE in capsys.readouterr().out


def test_zoom_is_zerospan_only(K, capsys):
    for mode in (["scan", "startFreq", "100e6", "endFreq", "104.8e6"], ["fmScan"], ["quickFullScan"], ["zeroSpanSave"]):
        with pytest.raises(SystemExit):
            K.handle_args({}, mode + ["zoom", "16"])
        assert "zeroSpan only" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        K.handle_args({}, ["zeroSpan", "bUsePSD", "true", "zoom", "16"])
    assert "bUsePSD false" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        K.handle_args({}, ["zeroSpan", "samplingRate", "2.4e6", "fftSize", "1048576", "frameBatch", "64", "zoom", "1024"])     # too long a batch
    assert K.ZOOM_RULE in capsys.readouterr().out
    d = K.handle_args({}, ["zeroSpanPlay", "fftSize", "512", "zoom", "16"])
    assert d["zoom.spec"] is None and "WARN" in capsys.readouterr().out
    assert d["endFreq"] - d["startFreq"] == d["samplingRate"]


def test_defaults_leave_the_reference_cases_alone(K):
    cli = json.load(open(os.path.join(GOLDEN, "cli_args.json")))
    for name, case in cli.items():
        d = K.handle_args({}, case["argv"] + ["prgLoopCnt", "0"])
        for k, want in case["d"].items():
            assert d[k] == want, (name, k)
        assert d["zoom.spec"] is None and d["zoom"] == ""


# ------------------------------------------------------------------------------------------ resources
def test_every_ddc_kernel_runs_without_scratch(tmp_path):
    kernels = _kernels(_asm(os.path.join(PKG_DIR, "csrc_ddc", "kdc_api.hip"), str(tmp_path / "kdc_api.s")))
    names = sorted(kernels)
    assert len([k for k in names if "tile_kernel<" in k]) == 12, names          # 4 formats x 4, 2, 1 outputs per thread
    assert len([k for k in names if "reduce_kernel<" in k]) == 4 and len([k for k in names if "history_kernel<" in k]) == 4, names
    assert len(names) == 20
    for k in names:
        assert _resource(kernels[k][1], "ScratchSize") == 0, k
