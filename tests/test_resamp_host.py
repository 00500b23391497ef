"""Host side of the resampler (no GPU needed): the companion header and library, the binding, the models every
GPU test compares against, the helpers, the `audioRate` key of the command line, and the kernels' resource report."""
import ctypes as C
import importlib
import json
import os
import re

import numpy as np
import pytest

import resamp_model as rm
from companion_helper import BY_MODULE, check_header_exports_binding
from conftest import GOLDEN, ROOT, load_pkg
from test_isa_regression import _asm, _kernels, _resource

PKG_DIR = os.path.join(ROOT, "prgs-sdr-kspecanal_amd")
PAIRS = [(3, 16), (147, 160), (160, 147), (1, 16), (24, 125), (3, 2), (2, 3), (1024, 1023), (1024, 1), (147, 800), (64, 1023), (5, 16)]
EMU_SHAPES = [(1, 1, 1), (1, 3, 4), (3, 1, 4), (2, 3, 5), (3, 2, 8), (147, 160, 12), (160, 147, 8), (1024, 1023, 8), (1024, 1, 16),
              (64, 1023, 256), (1, 16, 128)]


@pytest.fixture(scope="module")
def X():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.resamp")


@pytest.fixture(scope="module")
def K():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")


# ------------------------------------------------------------------------------------------ header, exports, binding
def test_header_is_c99_and_matches_the_exports_and_the_binding(X, tmp_path):
    text, _ = check_header_exports_binding(BY_MODULE["resamp"], X, tmp_path, "typedef krs_resamp* handle;\n",
                                           ["KRS_MAX_TAPS", "KRS_TYPE_C64", "KRS_OUT_S16", "(int)(KRS_MAX_POSITION >> 40)"])
    for name, value in (("KRS_MAX_L", X.MAX_L), ("KRS_MAX_M", X.MAX_M), ("KRS_MAX_RATIO", X.MAX_RATIO),
                        ("KRS_MAX_PHASE_TAPS", X.MAX_PHASE_TAPS), ("KRS_MAX_TAPS", X.MAX_TAPS), ("KRS_MAX_IN", X.MAX_IN),
                        ("KRS_MAX_POSITION", X.MAX_POSITION), ("KRS_TYPE_F32", X.TYPE_F32), ("KRS_TYPE_C64", X.TYPE_C64),
                        ("KRS_OUT_SAME", X.OUT_SAME), ("KRS_OUT_S16", X.OUT_S16)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value, name
    assert (X.TYPE_F32, X.TYPE_C64, X.OUT_SAME, X.OUT_S16) == (rm.TYPE_F32, rm.TYPE_C64, rm.OUT_SAME, rm.OUT_S16)
    assert X.MAX_IN == 2 ** 28 - 1 and X.MAX_POSITION == 2 ** 52


def test_the_other_bindings_hold_no_krs_name_and_the_package_exports_the_class(X):
    others = [importlib.import_module("prgs-sdr-kspecanal_amd." + m) for m in ("_lib", "density", "mask", "ddc", "detect", "demod", "chan")]
    assert not [n for m in others for n in m.SIGNATURES if n.startswith("krs_")]
    assert all(n.startswith("krs_") for n in X.SIGNATURES)
    pkg = load_pkg()
    for name in ("Resampler", "resample_taps", "rate_ratio"):
        assert getattr(pkg, name) is getattr(X, name) and name in pkg.__all__
    for name in ("process_dev", "process", "out_count", "blocks_dev", "block_out_count", "reset", "reset_at", "set_taps", "state",
                 "read_out", "kernel_info", "set_stream", "synchronize", "close"):
        assert callable(getattr(X.Resampler, name)), name
    assert isinstance(X.Resampler.out, property)
    companion = importlib.import_module("prgs-sdr-kspecanal_amd._companion")
    engine = importlib.import_module("prgs-sdr-kspecanal_amd.engine")
    assert issubclass(X.Resampler, companion.Companion) and isinstance(X._bind, companion.Binding) and X.DevArray is engine.DevArray


def test_library_loads_without_a_gpu_and_there_is_no_fallback(X):
    lib = X.load()
    assert lib.krs_abi_version() == X.ABI_VERSION
    try:
        import torch
        have_gpu = torch.cuda.is_available()
    except ImportError:
        have_gpu = False
    if not have_gpu:
        with pytest.raises(X.KsaError):
            X.Resampler(1, 1, np.ones(8, dtype=np.float32))
    missing = os.path.join(PKG_DIR, "no_such_libksa_resamp.so")
    with pytest.raises(X.KsaError) as e:
        X.load(missing)
    assert str(e.value) == ("libksa_resamp.so is missing at %s -- build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950); "
                            "there is no CPU fallback" % missing)
    with pytest.raises(X.KsaError, match=r"unknown type \[u8\]"):               # the binding's own refusals come before the library
        X.Resampler(1, 1, np.ones(8, dtype=np.float32), type="u8")
    with pytest.raises(X.KsaError, match=r"unknown out_fmt \[f16\]"):
        X.Resampler(1, 1, np.ones(8, dtype=np.float32), out_fmt="f16")
    with pytest.raises(X.KsaError, match="whole number of taps per phase"):
        X.Resampler(3, 2, np.ones(8, dtype=np.float32))
    # create-time refusals need no device: each has its own text and leaves a null handle
    taps = np.ones(16, dtype=np.float32)
    nan, inf = taps.copy(), taps.copy()
    nan[3], inf[5] = np.nan, np.inf
    big = np.ones(16384 + 1024, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    texts = []
    # (device, type, L, M, P, taps, out_fmt, pcm_scale, max_in)
    for args, text in (((0, 2, 2, 3, 8, p(taps), 0, 1.0, 64), "unknown sample type 2"), ((0, -1, 2, 3, 8, p(taps), 0, 1.0, 64), "unknown sample type -1"),
                       ((0, 0, 2, 3, 8, p(taps), 2, 1.0, 64), "unknown output format 2"), ((0, 0, 2, 3, 8, p(taps), -1, 1.0, 64), "unknown output format -1"),
                       ((0, 0, 0, 3, 8, p(taps), 0, 1.0, 64), "L 0 outside"), ((0, 0, 1025, 3, 8, p(big), 0, 1.0, 64), "L 1025 outside"),
                       ((0, 0, 2, 0, 8, p(taps), 0, 1.0, 64), "M 0 outside"), ((0, 0, 1024, 16385, 8, p(big), 0, 1.0, 64), "M 16385 outside"),
                       ((0, 0, 2, 33, 8, p(taps), 0, 1.0, 64), "M 33 exceeds 16 L = 32"),
                       ((0, 0, 4, 6, 4, p(taps), 0, 1.0, 64), "L / M = 4 / 6 is not reduced, use 2 / 3"),
                       ((0, 0, 2, 2, 8, p(taps), 0, 1.0, 64), "L / M = 2 / 2 is not reduced, use 1 / 1"),
                       ((0, 0, 2, 3, 0, p(taps), 0, 1.0, 64), "taps_per_phase 0 outside"), ((0, 0, 2, 3, 257, p(big), 0, 1.0, 64), "taps_per_phase 257 outside"),
                       ((0, 0, 1024, 1023, 17, p(big), 0, 1.0, 64), "17408 taps exceed 16384"),
                       ((0, 1, 2, 3, 8, p(taps), 1, 1.0, 64), "int16 output wants real input"),
                       ((0, 0, 2, 3, 8, p(taps), 0, 1.0, 0), "max_in 0 outside"), ((0, 0, 2, 3, 8, p(taps), 0, 1.0, 2 ** 28), "max_in 268435456 outside"),
                       ((0, 0, 2, 3, 8, None, 0, 1.0, 64), "null taps"), ((0, 0, 2, 3, 8, p(nan), 0, 1.0, 64), "tap 3 is not finite"),
                       ((0, 0, 2, 3, 8, p(inf), 0, 1.0, 64), "tap 5 is not finite"),
                       ((0, 0, 2, 3, 8, p(taps), 1, 0.0, 64), "pcm_scale 0"), ((0, 0, 2, 3, 8, p(taps), 1, -2.0, 64), "pcm_scale -2"),
                       ((0, 0, 2, 3, 8, p(taps), 1, np.inf, 64), "pcm_scale inf"), ((0, 0, 2, 3, 8, p(taps), 1, np.nan, 64), "pcm_scale nan"),
                       ((-1, 0, 2, 3, 8, p(taps), 0, 1.0, 64), "device -1")):
        h = C.c_void_p(1)
        assert lib.krs_create(*args, C.byref(h)) != 0 and h.value is None, text
        got = lib.krs_last_error().decode()
        assert text in got, (text, got)
        texts.append(re.sub(r"-?(inf|nan|[0-9][0-9.e+]*)", "#", got))
    # type / format / L / M / ratio / not reduced / P / T / s16 of complex / max_in / null taps / tap / pcm_scale / device
    assert len(set(texts)) == 14, sorted(set(texts))
    if not have_gpu:                                    # pcm_scale is only read for int16 output; only a device is missing then
        h = C.c_void_p(1)
        assert lib.krs_create(0, 0, 2, 3, 8, p(taps), 0, 0.0, 64, C.byref(h)) != 0 and h.value is None
        assert "hip" in lib.krs_last_error().decode()
    # a null object is refused by every entry point that takes one
    n = C.c_int64()
    calls = (lambda: lib.krs_out_count(None, 1, C.byref(n)), lambda: lib.krs_process_dev(None, None, 0, None, 0, None),
             lambda: lib.krs_process(None, None, 0, None, 0, None), lambda: lib.krs_blocks_dev(None, None, 0, 0, 0, None, 0),
             lambda: lib.krs_set_taps(None, None), lambda: lib.krs_reset(None), lambda: lib.krs_reset_at(None, 0),
             lambda: lib.krs_state(None, None, None), lambda: lib.krs_out_dev(None, None, None), lambda: lib.krs_read_out(None, None, 0, 0),
             lambda: lib.krs_kernel_info(None, None, None, None, None, None), lambda: lib.krs_set_stream(None, None),
             lambda: lib.krs_synchronize(None))
    for call in calls:
        assert call() != 0 and "null resampler" in lib.krs_last_error().decode()
    lib.krs_destroy(None)
    assert len(X.SIGNATURES) == len(calls) + 4          # those, abi_version, last_error, create, destroy


# ------------------------------------------------------------------------------------------ the model checks itself
def test_definition_equals_the_polyphase_form():
    rng = np.random.default_rng(11)
    for L, M, P, n in ((1, 1, 1, 9), (1, 3, 4, 40), (3, 1, 4, 17), (2, 3, 5, 41), (3, 2, 8, 33), (7, 5, 3, 50), (5, 16, 6, 70), (16, 5, 2, 11)):
        h = rng.standard_normal(L * P)
        for x in (rng.standard_normal(n), rng.standard_normal(n) + 1j * rng.standard_normal(n)):
            want = rm.definition(x, h, L, M)
            got = rm.polyphase(x, h, L, M)
            assert got.shape == want.shape == (rm.cdiv(n * L, M),)
            assert np.allclose(got, want, rtol=0, atol=1e-12)
    assert rm.definition(np.zeros(0), [1.0], 1, 1).shape == (0,) and rm.polyphase(np.zeros(0), [1.0], 1, 1).shape == (0,)


def test_out_count_over_random_cuts():
    rng = np.random.default_rng(12)
    for L, M in ((1, 1), (1, 3), (3, 1), (2, 3), (3, 2), (147, 160), (160, 147), (1024, 1023), (64, 1023), (1, 16)):
        at, total = 0, 0
        for c in rng.integers(0, 3 * M // L + 3, 200):
            k = rm.out_count(at, int(c), L, M)
            # the outputs whose newest sample n(m) = m M div L lies in [at, at + c)
            lo = rm.cdiv(at * L, M)
            ms = [m for m in range(max(0, lo - 2), lo + k + 2) if at <= (m * M) // L < at + int(c)]
            assert k == len(ms) and (not ms or ms[0] == lo), (L, M, at, c)
            at, total = at + int(c), total + k
        assert total == rm.cdiv(at * L, M)
    far = 2 ** 40 + 12345                                # Python ints: no overflow at far positions
    assert rm.out_count(far, 100, 1024, 1023) == (far + 100) * 1024 // 1023 - far * 1024 // 1023 + (
        ((far + 100) * 1024 % 1023 != 0) - (far * 1024 % 1023 != 0))


def test_block_first_and_count_keep_exactly_the_outputs_whose_support_lies_inside():
    for L, M, P in EMU_SHAPES + [(7, 5, 3), (5, 16, 6), (16, 5, 2)]:
        first = rm.block_first(L, M, P)
        assert first == 0 or ((first - 1) * M) // L < P - 1          # output first - 1 reaches in front of the block
        for block_len in sorted({P, P + 1, P + 7, 2 * P + 3, 4 * P + 100}):
            J = rm.block_out_count(block_len, L, M, P)
            if J < 1:                                                  # the first output past the transient needs a sample past the block
                assert J == 0 and (first * M) // L >= block_len and block_len < P + rm.cdiv(M, L)
                continue
            n =[((first + j) * M) // L for j in (0, J - 1)]
            assert P - 1 <= n[0] <= n[1] <= block_len - 1
            assert ((first + J) * M) // L >= block_len                 # the next one needs a sample past the block
        assert rm.block_out_count(P - 1, L, M, P) < 1
    rng = np.random.default_rng(13)
    L, M, P = 3, 2, 8
    h = rng.standard_normal(L * P)
    x = rng.standard_normal((2, 40))
    b = rm.blocks(x, h, L, M)
    first = rm.block_first(L, M, P)
    for row, got in zip(x, b):
        assert np.allclose(got, rm.definition(row, h, L, M)[first:], rtol=0, atol=1e-12)
    # a block that starts s = k M samples into a stream is the stream's outputs k L + first ...
    s = 3 * M
    stream = rm.definition(np.concatenate([rng.standard_normal(s), x[0]]), h, L, M)
    assert np.allclose(b[0], stream[3 * L + first:], rtol=0, atol=1e-12)


def test_exact_model_matches_the_float_model():
    rng = np.random.default_rng(14)
    for L, M, P in ((1, 1, 1), (2, 3, 5), (3, 2, 8), (7, 5, 3)):
        for kind in ("int", "pow2"):
            taps, num, den = rm.exact_taps(rng, L * P, kind)
            for cplx in (False, True):
                x = rm.exact_samples(rng, 50, cplx)
                want = rm.definition(x, taps, L, M)
                got = rm.exact_stream(x, num, den, L, M)
                assert got.dtype == (np.complex64 if cplx else np.float32) and np.array_equal(got, want)
                assert np.array_equal(rm.f32_at(x, taps, L, M, np.arange(len(want))), got)          # the float32 chain is exact too
            x = rm.exact_samples(rng, 50)
            assert np.array_equal(rm.exact_stream(x, num, den, L, M, rm.OUT_S16, 0.25), rm.pcm(rm.definition(x, taps, L, M), 0.25))
            bl, starts = 2 * P + 9, [0, 3, 2 * M]
            assert np.array_equal(rm.exact_blocks(x, num, den, L, M, starts, bl), rm.blocks(np.array([x[s:s + bl] for s in starts]), taps, L, M))
    # the int16 rule in integers: half to even, saturation at both ends
    num = np.array([1, 3, -1, -3, 5, 70000, -70000], dtype=np.int64)
    assert np.array_equal(rm.exact_pcm(num, 2, 1.0), [0, 2, 0, -2, 2, 32767, -32768])
    # far positions: t = m M in Python ints
    L, M, P = 1024, 1023, 8
    taps, num, den = rm.exact_taps(rng, L * P, "int")
    origin = 2 ** 40 + 12345
    x = rm.exact_samples(rng, 30)
    m0 = rm.cdiv(origin * L, M)
    ms = [m0 + j for j in range(rm.out_count(origin, 30, L, M))]
    got = rm.exact_at(x, num, den, L, M, ms, origin)
    want = [sum(int(num[(m * M) % L + q * L]) * (int(x[(m * M) // L - origin - q]) if (m * M) // L - origin - q >= 0 else 0) for q in range(P))
            for m in ms]
    assert np.array_equal(got, np.array(want, dtype=np.float32))


@pytest.mark.parametrize("shape", EMU_SHAPES, ids=str)
def test_float32_emulation_stays_inside_the_bound(X, shape):
    L, M, P = shape
    rng = np.random.default_rng(L * 7919 + M * 31 + P)
    taps = (rng.uniform(-1, 1, L * P) * np.hamming(L * P)).astype(np.float32)
    count = 600
    n = ((count - 1) * M) // L + 1
    ms = np.arange(count)
    for cplx in (False, True):
        x = rng.uniform(-1, 1, n).astype(np.float32)
        if cplx:
            x = (x + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)
        want = rm.at(x.astype(np.complex128 if cplx else np.float64), taps.astype(np.float64), L, M, ms)
        ratio = rm.worst_ratio(rm.f32_at(x, taps, L, M, ms), want, x, taps, L, M, ms)
        print("resampler emulation %s %s: error / bound %.4f" % (shape, "c64" if cplx else "f32", ratio))
        assert ratio <= 1.0, (shape, cplx, ratio)


# ------------------------------------------------------------------------------------------ the helpers
def _H(h, f):
    return abs(np.sum(h.astype(np.float64) * np.exp(-2j * np.pi * f * np.arange(len(h)))))


@pytest.mark.parametrize("pair", PAIRS, ids=str)
def test_resample_taps_properties(X, pair):
    L, M = pair
    W = max(L, M)
    for tpp in (8, 16):
        P = tpp * rm.cdiv(W, L)
        if P > X.MAX_PHASE_TAPS or L * P > X.MAX_TAPS:
            with pytest.raises(X.KsaError):
                X.resample_taps(L, M, tpp)
            continue
        h = X.resample_taps(L, M, tpp)
        assert h.dtype == np.float32 and h.shape == (L * P,)
        assert np.array_equal(h, h[::-1])
        h64 = h.astype(np.float64)
        assert abs(h64.sum() - L) <= 1e-6 * L
        assert np.max(np.abs(h64.reshape(P, L).sum(axis=0) - 1)) <= 2.5e-3
        assert abs(_H(h, 0.2 / W) / L - 1) <= 0.01
        for f in np.linspace(1.0 / W, min(W / 2, 8) / W, 57):
            assert _H(h, f) / L <= 2.5e-3, (pair, tpp, f)


def test_resample_taps_and_rate_ratio_limits(X):
    assert X.resample_taps(3, 16).shape == (3 * 8 * 6,) and X.resample_taps(147, 160, 12).shape == (147 * 24,)
    for bad in (lambda: X.resample_taps(0, 1), lambda: X.resample_taps(1025, 1), lambda: X.resample_taps(1, 17), lambda: X.resample_taps(3, 2, 0),
                lambda: X.resample_taps(1024, 1023, 17),    # 17408 taps
                lambda: X.resample_taps(1, 16, 17)):       # P = 272
        with pytest.raises(X.KsaError):
            bad()
    assert X.rate_ratio(256000, 48000) == (3, 16) and X.rate_ratio(240000, 44100) == (147, 800)
    assert X.rate_ratio(48000, 48000) == (1, 1) and X.rate_ratio(256000.0, 48000.0) == (3, 16)
    for bad in (lambda: X.rate_ratio(2.4e6 / 7, 48000), lambda: X.rate_ratio(48000, 44100.5), lambda: X.rate_ratio(0, 48000),
                lambda: X.rate_ratio(2400000, 48000 + 1), lambda: X.rate_ratio(1000000, 48000), lambda: X.rate_ratio("x", 1),
                lambda: X.rate_ratio(float("nan"), 1), lambda: X.rate_ratio(float("inf"), 1)):
        with pytest.raises(X.KsaError):
            bad()


# ------------------------------------------------------------------------------------------ command line
BASE = ["zeroSpan", "fftSize", "1024", "samplingRate", "2048000", "zoom", "8", "demod", "fm:1"]


def test_audiorate_key_parses(K, capsys):
    d = K.handle_args({}, BASE + ["audioRate", "48000"])
    dm = d["demod.spec"]
    assert sorted(dm) == sorted(["mode", "decim", "taps_per_phase", "ntaps", "deemph_us", "out_per_block", "rate"]) and dm["rate"] == 256000
    P = 8 * 6
    J = rm.block_out_count(dm["out_per_block"], 3, 16, P)
    assert d["resample.spec"] == dict(rate=48000, rate_in=256000, L=3, M=16, taps_per_phase=8, phase_taps=P,
                                      in_per_block=dm["out_per_block"], out_per_block=J)
    out = capsys.readouterr().out
    assert "WARN" not in out
    K.print_info(d)
    assert "INFO: audioRate [48000]: [256000] Hz -> [48000] Hz by L / M = [3] / [16], [%d] taps per phase, [%d] samples per block" % (P, J) \
        in capsys.readouterr().out
    s = K.handle_args({}, BASE + ["AUDIORATE", "44100:4"])["resample.spec"]
    assert (s["rate"], s["L"], s["M"], s["taps_per_phase"], s["phase_taps"]) == (44100, 441, 2560, 4, 4 * 6)
    s = K.handle_args({}, BASE[:-1] + ["fm:4", "audioRate", "48e3"])["resample.spec"]
    assert (s["rate"], s["rate_in"], s["L"], s["M"]) == (48000, 64000, 3, 4)
    # off: nothing but the new key's None
    d = K.handle_args({}, BASE)
    assert d["audioRate"] == "" and d["resample.spec"] is None and d["demod.spec"] == dm
    # the same chain without a whole rate in front keeps its WARN when the key is off
    capsys.readouterr()
    d = K.handle_args({}, ["zeroSpan", "fftSize", "1024", "zoom", "1", "demod", "fm:7"])
    assert "the audio rate [" in capsys.readouterr().out and d["resample.spec"] is None


@pytest.mark.parametrize("value", ["x", "0", "-48000", "48000.5", "nan", "inf", "48000:", "48000:0", "48000:x", "48000:8:1", ":", ":8",
                                   "48000:2.5", "1000:8",       # M = 256 > 16 L
                                   "255999",                    # L = 255999
                                   "48000:64"])                 # 6 x 64 taps per phase
def test_audiorate_key_refuses_with_the_rule(K, value, capsys):
    d = {}
    with pytest.raises(SystemExit):
        K.handle_args(d, BASE + ["audioRate", value])
    assert d["cmd.stop"] is True
    assert K.RESAMPLE_RULE in capsys.readouterr().out


def test_audiorate_is_zerospan_only_and_needs_demod_and_a_whole_rate(K, capsys):
    for mode in (["scan", "startFreq", "100e6", "endFreq", "104.8e6"], ["fmScan"], ["quickFullScan"], ["zeroSpanSave"]):
        with pytest.raises(SystemExit):
            K.handle_args({}, mode + ["audioRate", "48000"])
        assert "audioRate [48000] is zeroSpan only" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        K.handle_args({}, ["zeroSpan", "fftSize", "1024", "samplingRate", "2048000", "zoom", "8", "audioRate", "48000"])     # no demod
    out = capsys.readouterr().out
    assert "needs demod" in out and K.RESAMPLE_RULE in out
    with pytest.raises(SystemExit):
        K.handle_args({}, ["zeroSpan", "fftSize", "1024", "zoom", "1", "demod", "fm:7", "audioRate", "48000"])           # 2.4e6 / 7
    assert K.RESAMPLE_RULE in capsys.readouterr().out
    d = K.handle_args({}, ["zeroSpanPlay", "fftSize", "512", "zoom", "16", "demod", "fm", "audioRate", "48000"])
    assert d["resample.spec"] is None and "audioRate [48000] is ignored" in capsys.readouterr().out


def test_defaults_leave_the_reference_cases_alone(K):
    cli = json.load(open(os.path.join(GOLDEN, "cli_args.json")))
    for name, case in cli.items():
        d = K.handle_args({}, case["argv"] + ["prgLoopCnt", "0"])
        for k, want in case["d"].items():
            assert d[k] == want, (name, k)
        assert d["resample.spec"] is None and d["audioRate"] == ""


# ------------------------------------------------------------------------------------------ resources
def test_every_resampler_kernel_runs_without_scratch(tmp_path):
    kernels = _kernels(_asm(os.path.join(PKG_DIR, "csrc_resamp", "krs_api.hip"), str(tmp_path / "krs_api.s")))
    names = sorted(kernels)
    assert len([k for k in names if "tile_kernel<" in k]) == 6, names           # real x (float, int16) and complex, 4 and 1 outputs per thread
    assert len([k for k in names if "history_kernel<" in k]) == 2, names
    assert len(names) == 8
    for k in names:
        assert _resource(kernels[k][1], "ScratchSize") == 0, k
        assert _resource(kernels[k][1], "NumVgprs") <= 128, k
