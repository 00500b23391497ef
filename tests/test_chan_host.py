"""Host side of the polyphase channelizer (no GPU needed): the companion header and library, the binding, the models every GPU
test compares against, the helpers, the `channels` key of the command line, and the kernels' resource report."""
import ctypes as C
import importlib
import json
import os
import re

import numpy as np
import pytest

import chan_model as cm
from companion_helper import BY_MODULE, check_header_exports_binding
from conftest import GOLDEN, ROOT, load_pkg
from test_isa_regression import _asm, _kernels, _resource

PKG_DIR = os.path.join(ROOT, "prgs-sdr-kspecanal_amd")
GPU_SHAPES = [(2, 1, 1), (2, 2, 3), (4, 4, 2), (8, 2, 3), (16, 1, 4), (64, 4, 2), (32, 1, 32), (256, 2, 8), (512, 2, 16), (1024, 1, 8),
              (1024, 4, 8)]
SMALL_SHAPES = [(2, 1, 3), (4, 4, 2), (8, 2, 3), (16, 4, 2), (8, 1, 2)]


@pytest.fixture(scope="module")
def X():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.chan")


@pytest.fixture(scope="module")
def K():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")


# ------------------------------------------------------------------------------------------ header, exports, binding
def test_header_is_c99_and_matches_the_exports_and_the_binding(X, tmp_path):
    text, _ = check_header_exports_binding(BY_MODULE["chan"], X, tmp_path, "typedef kch_chan* handle;\n",
                                           ["KCH_MAX_TAPS", "KCH_FMT_S16", "KCH_FORM_LDS"])
    assert X.ABI_VERSION == X.load().kch_abi_version()
    for name, value in (("KCH_MIN_CHAN", X.MIN_CHAN), ("KCH_MAX_CHAN", X.MAX_CHAN), ("KCH_MAX_BRANCH_TAPS", X.MAX_BRANCH_TAPS),
                        ("KCH_MAX_TAPS", X.MAX_TAPS), ("KCH_MAX_IN", X.MAX_IN), ("KCH_FORM_LDS", X.FORM_LDS)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value, name
    pkg = load_pkg()
    assert [int(re.search(r"#define KCH_FMT_%s (\d+)" % n, text).group(1)) for n in ("C64", "U8", "S8", "S16")] == \
        [pkg.FMT_C64, pkg.FMT_U8, pkg.FMT_S8, pkg.FMT_S16] == [cm.FMT_C64, cm.FMT_U8, cm.FMT_S8, cm.FMT_S16]


def test_the_other_bindings_hold_no_kch_name_and_the_package_exports_the_class(X):
    others = [importlib.import_module("prgs-sdr-kspecanal_amd." + m) for m in ("_lib", "density", "mask", "ddc", "detect", "demod")]
    assert not [n for m in others for n in m.SIGNATURES if n.startswith("kch_")]
    assert all(n.startswith("kch_") for n in X.SIGNATURES)
    pkg = load_pkg()
    for name in ("Channelizer", "chan_prototype", "channel_freqs"):
        assert getattr(pkg, name) is getattr(X, name) and name in pkg.__all__
    for name in ("process_dev", "process", "out_count", "blocks_dev", "block_out_count", "block_len_for", "channel_power", "read_out",
                 "set_taps", "reset", "state", "kernel_info", "set_stream", "synchronize", "close"):
        assert callable(getattr(X.Channelizer, name)), name
    assert isinstance(X.Channelizer.out, property)


def test_library_loads_without_a_gpu_and_there_is_no_fallback(X):
    lib = X.load()
    assert lib.kch_abi_version() == X.ABI_VERSION
    try:
        import torch
        have_gpu = torch.cuda.is_available()
    except ImportError:
        have_gpu = False
    if not have_gpu:
        with pytest.raises(X.KsaError):
            X.Channelizer(cm.FMT_C64, 4, 2, np.ones(8, dtype=np.float32))
    with pytest.raises(X.KsaError, match="__graft_entry__"):
        X.load(os.path.join(PKG_DIR, "no_such_libksa_chan.so"))
    # create-time refusals need no device: each has its own text and leaves a null handle
    taps = np.ones(8192, dtype=np.float32)
    nan, inf = taps.copy(), taps.copy()
    nan[3], inf[5] = np.nan, np.inf
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    texts = []
    # (device, fmt, u8_offset, u8_scale, nchan, oversample, taps_per_branch, taps, max_in)
    for args, text in (((0, 0, 0.0, 1.0, 0, 1, 2, p(taps), 64), "nchan 0"), ((0, 0, 0.0, 1.0, 1, 1, 2, p(taps), 64), "nchan 1"),
                       ((0, 0, 0.0, 1.0, 12, 1, 2, p(taps), 64), "nchan 12"), ((0, 0, 0.0, 1.0, 2048, 1, 2, p(taps), 64), "nchan 2048"),
                       ((0, 0, 0.0, 1.0, 8, 0, 2, p(taps), 64), "oversample 0"), ((0, 0, 0.0, 1.0, 8, 3, 2, p(taps), 64), "oversample 3"),
                       ((0, 0, 0.0, 1.0, 8, 8, 2, p(taps), 64), "oversample 8"), ((0, 0, 0.0, 1.0, 2, 4, 2, p(taps), 64), "2 / 4"),
                       ((0, 0, 0.0, 1.0, 8, 2, 0, p(taps), 64), "taps_per_branch 0"), ((0, 0, 0.0, 1.0, 8, 2, 33, p(taps), 64), "taps_per_branch 33"),
                       ((0, 0, 0.0, 1.0, 1024, 2, 9, p(taps), 64), "9216 taps"),
                       ((0, 0, 0.0, 1.0, 8, 2, 2, p(taps), 0), "max_in 0"), ((0, 0, 0.0, 1.0, 8, 2, 2, p(taps), 2 ** 28), "max_in 268435456"),
                       ((0, 0, 0.0, 1.0, 8, 2, 2, None, 64), "null taps"), ((0, 0, 0.0, 1.0, 8, 2, 2, p(nan), 64), "tap 3 is not finite"),
                       ((0, 0, 0.0, 1.0, 8, 2, 2, p(inf), 64), "tap 5 is not finite"),
                       ((0, 4, 0.0, 1.0, 8, 2, 2, p(taps), 64), "unknown sample format 4"), ((0, -1, 0.0, 1.0, 8, 2, 2, p(taps), 64), "unknown sample format -1"),
                       ((0, 1, 0.0, 0.0, 8, 2, 2, p(taps), 64), "u8_scale 0"), ((0, 1, 0.0, np.inf, 8, 2, 2, p(taps), 64), "u8_scale inf"),
                       ((0, 1, np.nan, 1.0, 8, 2, 2, p(taps), 64), "u8_offset nan"), ((-1, 0, 0.0, 1.0, 8, 2, 2, p(taps), 64), "device -1")):
        h = C.c_void_p(1)
        assert lib.kch_create(*args, C.byref(h)) != 0 and h.value is None, text
        got = lib.kch_last_error().decode()
        assert text in got, (text, got)
        texts.append(re.sub(r"-?(inf|nan|[0-9][0-9.e+]*)", "#", got))
    # nchan / oversample / decimation / taps_per_branch / prototype / max_in / null taps / tap / format / u8_scale / u8_offset / device
    assert len(set(texts)) == 12, sorted(set(texts))
    if not have_gpu:                                    # a zero u8_scale is only read for uint8 input; only a device is missing then
        h = C.c_void_p(1)
        assert lib.kch_create(0, 0, 0.0, 0.0, 8, 2, 2, p(taps), 64, C.byref(h)) != 0 and h.value is None
        assert "hip" in lib.kch_last_error().decode()
    # a null object is refused by every entry point that takes one, before any HIP call
    n = C.c_int64()
    for call in (lambda: lib.kch_out_count(None, 1, C.byref(n)), lambda: lib.kch_process_dev(None, None, 0, None, 0, None),
                 lambda: lib.kch_process(None, None, 0, None, 0, None), lambda: lib.kch_blocks_dev(None, None, 0, 0, 0, None, 0),
                 lambda: lib.kch_channel_power(None, 0, 0, None), lambda: lib.kch_set_taps(None, None), lambda: lib.kch_reset(None),
                 lambda: lib.kch_state(None, None, None), lambda: lib.kch_out_dev(None, None, None, None, None),
                 lambda: lib.kch_read_out(None, None, 0, 0, 0), lambda: lib.kch_kernel_info(None, None, None, None, None, None, None),
                 lambda: lib.kch_set_stream(None, None), lambda: lib.kch_synchronize(None)):
        assert call() != 0 and "null channelizer" in lib.kch_last_error().decode()
    lib.kch_destroy(None)


# ------------------------------------------------------------------------------------------ the model checks itself
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=str)
def test_polyphase_evaluation_equals_the_definition(shape):
    M, O, P = shape
    rng = np.random.default_rng(M * 100 + O * 10 + P)
    n = 7 * M + 3
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    h = rng.standard_normal(M * P)
    want = cm.definition(x, h, M, O)
    got = cm.polyphase(x, h, M, O)
    assert got.shape == want.shape == (M, -(-n // (M // O)))
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))
    # and the definition is the down-converter's: mix by exp(-2 pi i c n / M), filter, keep every D-th
    for c in (1, M // 2, M - 1):
        v = x * np.exp(-2j * np.pi * ((c * np.arange(n)) % M) / M)
        assert np.allclose(np.convolve(v, h)[:n:M // O], want[c], rtol=0, atol=1e-12 * np.max(np.abs(want)))


@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=str)
def test_block_count_formula_against_brute_force(shape):
    """A block's columns are the stream's columns m whose support [m D - (T - 1), m D] lies inside the block."""
    M, O, P = shape
    D, T = M // O, M * P
    first = cm.first_column(M, O, P)
    assert first == (O * P if D > 1 else T - 1)
    for L in range(1, 4 * D + T + 1):
        brute = [m for m in range(L) if m * D - (T - 1) >= 0 and m * D <= L - 1]
        if L < first * D + 1:
            assert not brute and cm.block_out_count(L, M, O, P) <= 0, (shape, L)
        else:
            assert brute == list(range(first, first + cm.block_out_count(L, M, O, P))), (shape, L)
    for F in (1, 2, 17):
        assert cm.block_out_count(cm.block_len_for(F, M, O, P), M, O, P) == F
        assert cm.block_out_count(cm.block_len_for(F, M, O, P) - 1, M, O, P) == F - 1


def test_out_count_over_random_cuts():
    rng = np.random.default_rng(7)
    for D in (1, 2, 8, 256, 1024):
        at, total = 0, 0
        for c in rng.integers(0, 3 * D + 2, 200):
            k = cm.out_count(at, int(c), D)
            assert k == len(range(-(-at // D) * D, at + int(c), D))
            at, total = at + int(c), total + k
        assert total == -(-at // D)


def test_integer_model_matches_the_float_model_on_the_axis_channels():
    rng = np.random.default_rng(8)
    M, O, P, n = 8, 2, 3, 90
    taps = rng.integers(-3, 4, M * P)
    for fmt, raw in ((cm.FMT_S16, rng.integers(-32768, 32768, 2 * n).astype(np.int16)), (cm.FMT_S8, rng.integers(-128, 128, 2 * n).astype(np.int8)),
                     (cm.FMT_U8, rng.integers(0, 256, 2 * n).astype(np.uint8)),
                     (cm.FMT_C64, ((rng.integers(-999, 999, n) + 1j * rng.integers(-999, 999, n)) / 32768).astype(np.complex64))):
        iq, scale = cm.to_int(raw, fmt)
        want = cm.definition(cm.unpack(raw, fmt, 128.0, 128.0), taps, M, O)
        cols = np.arange(want.shape[1])
        for c in (0, 2, 4, 6):
            assert np.allclose(cm.int_channel(iq, scale, taps, M, O, c, cols), want[c], rtol=0, atol=1e-5), (fmt, c)
        emu = cm.f32_polyphase(cm.unpack(raw, fmt, 128.0, 128.0).astype(np.complex64), taps, M, O, cols)
        for c in (0, 2, 4, 6):                          # the float32 network is exact there, as the GPU test asks of the kernel
            assert np.array_equal(emu[c], cm.int_channel(iq, scale, taps, M, O, c, cols)), (fmt, c)


EMU_WORST = {}


@pytest.mark.parametrize("shape", GPU_SHAPES, ids=str)
def test_float32_emulation_stays_inside_the_bound(X, shape):
    """The premise of the GPU float test: the float32 emulation of the evaluation (chains of fused multiply-adds, the radix-2
    network with rounded products) stays inside (P + 4 log2 M + 16) 2^-24 sum|h| max|x| at every GPU shape.  The worst fraction is
    printed, not fixed in advance (DESIGN 4.16 records it)."""
    M, O, P = shape
    D, T = M // O, M * P
    taps = X.chan_prototype(M, P)
    cols = np.arange(40)
    n = D * 39 + 1
    rng = np.random.default_rng(M * 31337 + O * 7 + P)
    x = (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)
    want = cm.polyphase(x.astype(np.complex128), taps, M, O, cols)
    emu = cm.f32_polyphase(x, taps, M, O, cols)
    ratio = float(np.max(np.abs(emu - want)) / cm.bound(taps, np.abs(x).max(), M, P))
    EMU_WORST[shape] = ratio
    print("chan emulation %s: worst error / bound = %.4f" % (shape, ratio))
    assert ratio <= 1.0, ratio


def test_twiddles_are_exact_on_the_axes():
    for M in (2, 4, 8, 64, 1024):
        re, im = cm.twiddles(M)
        assert (re[0], im[0]) == (1, 0) and re.dtype == np.float32 and len(re) == max(M // 2, 1)
        if M >= 4:
            assert (re[M // 4], im[M // 4]) == (0, 1)
        k = np.arange(len(re))
        assert np.max(np.abs((re + 1j * im) - np.exp(2j * np.pi * k / M))) <= 2.0 ** -24


def test_plan_keeps_every_shape_inside_the_lds(X):
    for M in (2 ** k for k in range(1, 11)):
        for O in (1, 2, 4):
            for P in range(1, 33):
                if M // O < 1 or M * P > X.MAX_TAPS:
                    continue
                W, pitch, lds, threads = cm.plan(M, O, P)
                assert W >= 1 and W & (W - 1) == 0 and W * M <= 8192 and lds <= 160 * 1024 and threads * (160 * 1024 // lds) >= 1024, (M, O, P, W, lds)
    assert cm.plan(256, 2, 8)[0] == 16 and cm.plan(256, 2, 8)[2] <= 80 * 1024
    assert cm.plan(1024, 1, 8)[0] == 4


# ------------------------------------------------------------------------------------------ the helpers
def test_chan_prototype_has_dc_gain_one_and_is_symmetric(X):
    for M, P, cutoff, window in ((2, 1, 1.0, "hamming"), (4, 8, 1.0, "hamming"), (16, 8, 0.8, "hamming"), (64, 16, 1.0, "hanning"),
                                 (1024, 8, 1.0, "hamming"), (256, 32, 0.8, "hamming")):
        h = X.chan_prototype(M, P, cutoff, window)
        assert h.dtype == np.float32 and h.shape == (M * P,) and abs(float(h.astype(np.float64).sum()) - 1) < 1e-6
        assert np.array_equal(h, h[::-1])
        if P < 4:
            continue
        grid = 8 * M * P
        H = np.abs(np.fft.rfft(h.astype(np.float64), grid))
        first_below = int(np.argmax(H < 0.5))            # the -6 dB point, in grid steps
        assert abs(first_below - cutoff * grid / (2 * M)) <= 2, (M, P, cutoff, first_below)
    for bad in (lambda: X.chan_prototype(1), lambda: X.chan_prototype(12), lambda: X.chan_prototype(2048), lambda: X.chan_prototype(1024, 9),
                lambda: X.chan_prototype(8, 33), lambda: X.chan_prototype(8, 8, 0.0)):
        with pytest.raises(X.KsaError):
            bad()


def test_channel_freqs_put_the_upper_half_below_the_centre(X):
    f = X.channel_freqs(8, 2.4e6, 100e6)
    assert f.shape == (8,) and np.array_equal(f, 100e6 + np.array([0, 1, 2, 3, -4, -3, -2, -1]) * 300e3)
    assert np.array_equal(X.channel_freqs(2, 2.0), [0.0, -1.0])


# ------------------------------------------------------------------------------------------ command line
def test_channels_key_parses_in_each_form(K):
    base = ["zeroSpan", "fftSize", "1024", "channels"]
    d = K.handle_args({}, base + ["16"])
    full, fs, fc = d["fullSize"], d["samplingRate"], d["centerFreq"]
    assert d["chan.spec"] == dict(nchan=16, oversample=2, taps_per_branch=8, pick=0, decim=8, ntaps=128, first=16,
                                  block_len=8 * (16 + full - 1) + 1, offset=0.0, center=fc, span=fs / 8)
    assert (d["startFreq"], d["endFreq"]) == (fc - fs / 16, fc + fs / 16) and d["zoom.spec"] is None
    s = K.handle_args({}, base + ["16:1"])["chan.spec"]
    assert (s["oversample"], s["decim"], s["first"], s["span"]) == (1, 16, 8, fs / 16)
    s = K.handle_args({}, base + ["8:2:4:3"])["chan.spec"]
    assert (s["nchan"], s["decim"], s["ntaps"], s["pick"], s["offset"], s["center"]) == (8, 4, 32, 3, 3 * fs / 8, fc + 3 * fs / 8)
    s = K.handle_args({}, base + ["8:4:4:5"])["chan.spec"]
    assert (s["decim"], s["first"], s["offset"]) == (2, 16, -3 * fs / 8)
    s = K.handle_args({}, base + ["2:2:3:1"])["chan.spec"]
    assert (s["decim"], s["first"], s["block_len"], s["offset"]) == (1, 5, 5 + full, -fs / 2)
    d = K.handle_args({}, ["zeroSpan", "fftSize", "1024", "iqFormat", "s16", "frameBatch", "4", "channels", "16:2:8:3", "demod", "fm:5:8:75",
                           "density", "64:-120:0", "detect", "8:2:6"])       # it combines with the other keys, and satisfies demod
    assert d["chan.spec"]["pick"] == 3 and d["density.spec"] and d["detect.spec"]
    assert d["demod.spec"]["rate"] == int(round(fs / (8 * 5))) and d["demod.spec"]["mode"] == "fm"
    d = K.handle_args({}, ["zeroSpan", "fftSize", "1024"])
    assert d["channels"] == "" and d["chan.spec"] is None and d["channelsSave"] == ""


@pytest.mark.parametrize("value", ["x", "0", "1", "12", "2048", "-4", "2.5", "16:", "16:3", "16:0", "16:8", "2:4", "16:2:0", "16:2:33", "1024:2:9",
                                   "16:2:8:16", "16:2:8:-1", "16:2:8:x", "16:2:8:3:1", ":", "16:2:2.5"])
def test_channels_key_refuses_with_the_rule(K, value, capsys):
    d = {}
    with pytest.raises(SystemExit):
        K.handle_args(d, ["zeroSpan", "fftSize", "1024", "channels", value])
    assert d["cmd.stop"] is True
    assert K.CHANNELS_RULE in capsys.readouterr().out


def test_channels_is_zerospan_only_and_excludes_zoom(K, capsys):
    for mode in (["scan", "startFreq", "100e6", "endFreq", "104.8e6"], ["fmScan"], ["quickFullScan"], ["zeroSpanSave"]):
        with pytest.raises(SystemExit):
            K.handle_args({}, mode + ["channels", "16"])
        assert "zeroSpan only" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        K.handle_args({}, ["zeroSpan", "bUsePSD", "true", "channels", "16"])
    assert "bUsePSD false" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        K.handle_args({}, ["zeroSpan", "zoom", "4", "channels", "16"])
    assert "exclude each other" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        K.handle_args({}, ["zeroSpan", "samplingRate", "2.4e6", "fftSize", "1048576", "frameBatch", "64", "channels", "1024:1"])   # too long a batch
    assert K.CHANNELS_RULE in capsys.readouterr().out
    d = K.handle_args({}, ["zeroSpanPlay", "fftSize", "512", "channels", "16"])
    assert d["chan.spec"] is None and "WARN" in capsys.readouterr().out
    assert d["endFreq"] - d["startFreq"] == d["samplingRate"]
    d = K.handle_args({}, ["zeroSpan", "fftSize", "512", "channelsSave", "x.npz"])
    assert d["chan.spec"] is None and "channelsSave [x.npz] is ignored without channels" in capsys.readouterr().out
    with pytest.raises(SystemExit):                      # demod still needs a front end, and says so in its own words
        K.handle_args({}, ["zeroSpan", "fftSize", "512", "demod", "fm"])
    assert K.DEMOD_RULE in capsys.readouterr().out


def test_defaults_leave_the_reference_cases_alone(K):
    cli = json.load(open(os.path.join(GOLDEN, "cli_args.json")))
    for name, case in cli.items():
        d = K.handle_args({}, case["argv"] + ["prgLoopCnt", "0"])
        for k, want in case["d"].items():
            assert d[k] == want, (name, k)
        assert d["chan.spec"] is None and d["channels"] == ""


# ------------------------------------------------------------------------------------------ resources
def test_every_chan_kernel_runs_without_scratch_and_inside_the_lds(tmp_path):
    kernels = _kernels(_asm(os.path.join(PKG_DIR, "csrc_chan", "kch_api.hip"), str(tmp_path / "kch_api.s")))
    names = sorted(kernels)
    assert len([k for k in names if "chan_kernel<" in k]) == 4 and len([k for k in names if "history_kernel<" in k]) == 4, names
    assert len([k for k in names if "power_kernel" in k]) == 1 and len(names) == 9, names
    for k in names:
        assert _resource(kernels[k][1], "ScratchSize") == 0, k
        assert _resource(kernels[k][1], "LDSByteSize") == 0, k          # all LDS is dynamic: the plan's, checked above to stay at 160 KiB
