"""Host side of the IQ corrector (no GPU needed): the model every GPU test compares against on hand-worked cases and on the
definition's purpose, the companion header and library, the binding, and the `iqfix` / `iqfixSave` keys of the
command line."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import iqfix_model as qm
from companion_helper import BY_MODULE, check_header_exports_binding
from conftest import ROOT, load_pkg

PKG_DIR = os.path.join(ROOT, "prgs-sdr-kspecanal_amd")
LIB = os.path.join(PKG_DIR, "libksa_iqfix.so")
SRC_DIR = os.path.join(PKG_DIR, "csrc_iqfix")
F32 = np.float32


@pytest.fixture(scope="module")
def X():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.iqfix")


@pytest.fixture(scope="module")
def K():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")


# ------------------------------------------------------------------------------------------ the model on hand-worked cases
def test_quantities_round_ties_to_even():
    # k 2^-31 for odd k: times 2^30 it is k / 2, a tie, which goes to the even neighbour
    k = np.array([1, 3, 5, 7, -1, -3, -5, 2 ** 20 + 1], dtype=np.float64)
    x = (k * 2.0 ** -31).astype(F32)
    want = [0, 2, 2, 4, 0, -2, -2, 2 ** 19]
    a_i, a_q, c_ii, c_qq, c_iq = qm.quantities(x, x[::-1].copy())
    assert list(a_i) == want and list(a_q) == want[::-1]
    # products that are ties: 2^-15 x 3 2^-16 = 3 2^-31 -> 2; (2^-16 x 3)(2^-15 x 5)= 15 2^-31 -> 8; squares: (3 2^-16)^2 = 9 2^-32 -> 2.25 -> 2
    xr = np.array([2.0 ** -15, 3 * 2.0 ** -16, -(2.0 ** -15)], dtype=F32)
    xi = np.array([3 * 2.0 ** -16, 5 * 2.0 ** -15, 2.0 ** -16], dtype=F32)
    _, _, c_ii, c_qq, c_iq = qm.quantities(xr, xi)
    assert list(c_iq) == [2, 8, 0] and list(c_ii) == [1, 2, 1] and list(c_qq) == [2, 25, 0]


def test_quantities_saturate_at_four():
    xr = np.array([4, 5, -4, -7, 2, 3, 3, -3, 1e30, 0.5], dtype=F32)
    xi = np.array([0, 0, 0, 0, 2, -3, 3, -3, -1e30, -0.25], dtype=F32)
    a_i, a_q, c_ii, c_qq, c_iq = qm.quantities(xr, xi)
    T = 2 ** 32
    assert list(a_i) == [T, T, -T, -T, 2 ** 31, 3 * 2 ** 30, 3 * 2 ** 30, -3 * 2 ** 30, T, 2 ** 29]
    assert list(a_q) == [0, 0, 0, 0, 2 ** 31, -3 * 2 ** 30, 3 * 2 ** 30, -3 * 2 ** 30, -T, -2 ** 28]
    assert list(c_ii) == [T, T, T, T, T, T, T, T, T, 2 ** 28]
    assert list(c_qq) == [0, 0, 0, 0, T, T, T, T, T, 2 ** 26]
    assert list(c_iq) == [0, 0, 0, 0, T, -T, T, T, -T, -2 ** 27]
    s = qm.stats(xr, xi)
    assert s.dtype == np.int64 and s[5] == 10 and s[2] == 9 * T + 2 ** 28
    # the integer formats: full scale and the asymmetric end
    s16 = np.array([[-32768, 32767], [16384, -16384]], dtype=np.int16)
    a_i, a_q, c_ii, c_qq, c_iq = qm.quantities(*qm.unpack(s16, "s16"))
    assert list(a_i) == [-2 ** 30, 2 ** 29] and list(a_q) == [32767 * 2 ** 15, -2 ** 29]
    assert list(c_ii) == [2 ** 30, 2 ** 28] and list(c_iq) == [-32767 * 2 ** 15, -2 ** 28]
    assert list(qm.quantities(*qm.unpack(np.array([[255, 0]], dtype=np.uint8), "u8"))[0]) == [2 ** 30]
    assert list(qm.quantities(*qm.unpack(np.array([[-128, 64]], dtype=np.int8), "s8"))[1]) == [2 ** 29]
    xr, xi = qm.unpack(np.array([[200, 100]], dtype=np.uint8), "u8", 100.0, 50.0)
    assert (xr[0], xi[0]) == (F32(100.0) * (F32(1) / F32(50.0)), F32(0))


def test_solve_by_hand_and_its_flags():
    # empty
    sol = qm.solve(np.zeros(6, dtype=np.int64), 3)
    assert (sol["flags"], sol["count"], qm.coeffs_of(sol)) == (qm.FLAG_EMPTY, 0, qm.IDENTITY)
    assert qm.solve(qm.stats(np.zeros(0, F32), np.zeros(0, F32)), 1)["flags"] == qm.FLAG_EMPTY
    # a constant: the means are the constant, no variance -> DEGENERATE under IQ, nothing flagged under DC alone
    xr, xi = np.full(64, 0.25, F32), np.full(64, -0.5, F32)
    sol = qm.solve(qm.stats(xr, xi), 3)
    assert (sol["dc_i"], sol["dc_q"], sol["c"], sol["d"], sol["flags"], sol["count"]) == (0.25, -0.5, 0, 1, qm.FLAG_DEGENERATE, 64)
    sol = qm.solve(qm.stats(xr, xi), qm.MODE_DC)
    assert (sol["dc_i"], sol["dc_q"], sol["c"], sol["d"], sol["flags"]) == (0.25, -0.5, 0, 1, 0)
    assert qm.solve(qm.stats(xr, xi), qm.MODE_IQ)["dc_i"] == 0
    # I alone: vQQ = 0, so w = 0 -> DEGENERATE
    xr = np.array([0.5, -0.5] * 8, dtype=F32)
    sol = qm.solve(qm.stats(xr, np.zeros(16, F32)), 3)
    assert (sol["c"], sol["d"], sol["flags"]) == (0, 1, qm.FLAG_DEGENERATE)
    # a clean pair: I = (+-0.5), Q = 0.25 of an uncorrelated pattern -> d = 2, c = 0
    xr = np.array([0.5, 0.5, -0.5, -0.5], dtype=F32)
    xi = np.array([0.25, -0.25, 0.25, -0.25], dtype=F32)
    sol = qm.solve(qm.stats(xr, xi), 3)
    assert qm.coeffs_of(sol) == (0, 0, 0, 2) and sol["flags"] == 0
    # Q = 0.5 I + that pattern: r = vIQ / vII = 0.5, w = 0.0625, d = 2, c = -1
    sol = qm.solve(qm.stats(xr, (F32(0.5) * xr + xi).astype(F32)), 3)
    assert qm.coeffs_of(sol) == (0, 0, -1, 2) and sol["flags"] == 0
    y = qm.apply(xr, (F32(0.5) * xr + xi).astype(F32), qm.coeffs_of(sol))
    assert np.array_equal(y, (xr + 2j * xi).astype(np.complex64))
    # the ratio guard at both ends: count 1, no mean, vII / w = sums[2] / sums[3]
    for c_ii, c_qq, d, flags in ((2 ** 30, 2 ** 22, 16.0, 0), (2 ** 30, 2 ** 22 - 1, 1.0, qm.FLAG_DEGENERATE),
                                 (2 ** 22, 2 ** 30, 0.0625, 0), (2 ** 22 - 1, 2 ** 30, 1.0, qm.FLAG_DEGENERATE)):
        sol = qm.solve([0, 0, c_ii, c_qq, 0, 1], qm.MODE_IQ)
        assert (sol["d"], sol["c"], sol["flags"]) == (d, 0, flags), (c_ii, c_qq)
    # apply: the identity gives the input; every step is a float32 step
    x = (np.arange(8) / 7 - 0.3).astype(F32)
    assert np.array_equal(qm.apply(x, -x), (x - 1j * x).astype(np.complex64))
    y = qm.apply(x, -x, (0.1, -0.2, 0.3, 0.9))
    ui, uq = x - F32(0.1), -x - F32(-0.2)
    assert np.array_equal(y.real, ui) and np.array_equal(y.imag, F32(0.3) * ui + F32(0.9) * uq)
    g, p = qm.imbalance_of(-np.sin(np.radians(5.0)) / 1.1, np.cos(np.radians(5.0)) / 1.1)    # a Q row of length 1 / 1.1, tilted by 5 degrees
    assert abs(g - 20 * np.log10(1.1)) < 1e-12 and abs(p - 5.0) < 1e-12


@pytest.mark.parametrize("n, image_gain, dc_gain", [(65536, 47.8, 55.5), (4096, 37.6, 41.8)])
def test_the_definition_removes_the_image_and_the_dc_spike(n, image_gain, dc_gain):
    """An s16 capture of a tone of amplitude 0.3 at bin n/8 plus noise of sigma 0.01, with 1 dB and 5 degrees of imbalance and a
    DC offset of (0.05, -0.03), solved with dc+iq from its own sums and corrected.  Measured with this model and its seed, over 5
    bins each under a hanning window:

        length   image rejection        DC rejection
        65536    22.79 dB -> 70.56 dB   14.74 dB -> 70.20 dB     (improvements 47.8 and 55.5 dB)
        4096     22.74 dB -> 60.35 dB   14.72 dB -> 56.52 dB     (improvements 37.6 and 41.8 dB)

    The assertion is an improvement of at least those figures minus 10 dB.  dc alone leaves the image where it was and iq alone
    the spike."""
    xr, xi = qm.unpack(qm.impaired_capture(n), "s16")
    image0, dc0 = qm.rejections(xr + 1j * xi)
    sol = qm.solve(qm.stats(xr, xi), qm.MODE_DC | qm.MODE_IQ)
    assert sol["flags"] == 0 and sol["count"] == n
    image1, dc1 = qm.rejections(qm.apply(xr, xi, qm.coeffs_of(sol)))
    print("n %d: image %.2f -> %.2f dB, dc %.2f -> %.2f dB" % (n, image0, image1, dc0, dc1))
    assert image1 - image0 >= image_gain - 10.0 and dc1 - dc0 >= dc_gain - 10.0
    assert abs(image0 - 22.8) < 0.2 and abs(dc0 - 14.7) < 0.2
    image_dc, dc_dc = qm.rejections(qm.apply(xr, xi, qm.coeffs_of(qm.solve(qm.stats(xr, xi), qm.MODE_DC))))
    assert abs(image_dc - image0) < 0.1 and dc_dc - dc0 >= dc_gain - 10.0
    image_iq, dc_iq = qm.rejections(qm.apply(xr, xi, qm.coeffs_of(qm.solve(qm.stats(xr, xi), qm.MODE_IQ))))
    assert image_iq - image0 >= image_gain - 10.0 and abs(dc_iq - dc0) < 1.0
    g, p = qm.imbalance_of(sol["c"], sol["d"])
    assert abs(g - 0.93) < 0.05 and abs(p - 5.6) < 0.1


# ------------------------------------------------------------------------------------------ header, exports, binding
def _ctype_of(X, param):
    p = " ".join(param.split())
    if p == "void":
        return None
    if "**" in p:
        return C.POINTER(C.c_void_p)
    if p.startswith("kqf_coeffs*"):
        return C.POINTER(X.Coeffs)
    if p.startswith(("kqf_corrector*", "const void*", "void*")):
        return C.c_void_p
    if p.startswith("int64_t") and "[" in p:
        return C.POINTER(C.c_int64)
    if p.startswith("int32_t*"):
        return C.POINTER(C.c_int32)
    for name, t in (("int32_t ", C.c_int32), ("int64_t ", C.c_int64), ("float ", C.c_float)):
        if p.startswith(name):
            return t
    raise AssertionError(p)


def test_header_is_c99_and_matches_the_exports_and_the_binding(X, tmp_path):
    extra = ('typedef kqf_corrector* handle;\ntypedef char coeffs_are_32_bytes[sizeof(kqf_coeffs) == 32 ? 1 : -1];\n'
             + "".join('typedef char %s_at_%d[offsetof(kqf_coeffs, %s) == %d ? 1 : -1];\n' % (f, o, f, o)
                       for f, o in (("dc_i", 0), ("dc_q", 4), ("c", 8), ("d", 12), ("flags", 16), ("mode", 20), ("count", 24))))
    text, names = check_header_exports_binding(BY_MODULE["iqfix"], X, tmp_path, extra,
                                               ["KQF_FMT_S16", "KQF_MAX_IN", "KQF_MODE_DC", "KQF_MODE_IQ", "KQF_FLAG_DEGENERATE",
                                                "KQF_FLAG_EMPTY"])
    protos = re.findall(r"^(int|void|const char\*) (kqf_[a-z0-9_]+)\((.*?)\);", text, re.M | re.S)
    assert names == sorted(n for _, n, _ in protos)                # every name the header holds is a declaration of this shape
    assert names == sorted(set(re.findall(r"\b(kqf_[a-z0-9_]+)\s*\(", text.split("#ifndef KSA_IQFIX_H")[1])))
    # the binding's signatures are the header's declarations, argument by argument
    for ret, name, params in protos:
        res, args = X.SIGNATURES[name]
        assert res == {"int": C.c_int, "void": None, "const char*": C.c_char_p}[ret], name
        want = [t for t in (_ctype_of(X, p) for p in params.split(",")) if t is not None]
        assert args == want, (name, args, want)
    # constants
    for name, value in (("KQF_ABI_VERSION", X.ABI_VERSION), ("KQF_MAX_IN", X.MAX_IN), ("KQF_MAX_COUNT", X.MAX_COUNT),
                        ("KQF_UNIT", X.UNIT), ("KQF_MODE_DC", X.MODE_DC), ("KQF_MODE_IQ", X.MODE_IQ),
                        ("KQF_FLAG_DEGENERATE", X.FLAG_DEGENERATE), ("KQF_FLAG_EMPTY", X.FLAG_EMPTY), ("KQF_FMT_C64", X.FMT_C64),
                        ("KQF_FMT_U8", X.FMT_U8), ("KQF_FMT_S8", X.FMT_S8), ("KQF_FMT_S16", X.FMT_S16)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value, name
    assert X.ABI_VERSION == 1 and X.MAX_IN == 2 ** 28 - 1 and X.MAX_COUNT == 2 ** 30 == qm.MAX_COUNT and X.UNIT == 2 ** 30 == qm.UNIT
    assert (X.MODE_DC, X.MODE_IQ, X.FLAG_DEGENERATE, X.FLAG_EMPTY) == (qm.MODE_DC, qm.MODE_IQ, qm.FLAG_DEGENERATE, qm.FLAG_EMPTY) == (1, 2, 1, 2)
    assert X.MODES == {"dc": 1, "iq": 2, "dc+iq": 3}
    ddc = importlib.import_module("prgs-sdr-kspecanal_amd.ddc")
    assert (X.FMT_C64, X.FMT_U8, X.FMT_S8, X.FMT_S16) == (ddc.FMT_C64, ddc.FMT_U8, ddc.FMT_S8, ddc.FMT_S16) == (0, 1, 2, 3)
    fields = re.search(r"typedef struct kqf_coeffs \{(.*?)\} kqf_coeffs;", text, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    listed = [n.strip() for decl in re.findall(r"(?:float|int32_t|int64_t)\s+([\w,\s]+);", fields) for n in decl.split(",")]
    assert listed == [n for n, _ in X.Coeffs._fields_] and C.sizeof(X.Coeffs) == 32


def test_the_other_bindings_hold_no_kqf_name_and_the_package_exports_the_class(X):
    others = [importlib.import_module("prgs-sdr-kspecanal_amd." + m)
              for m in ("_lib", "density", "mask", "ddc", "detect", "demod", "chan", "resamp", "corr", "pulse", "track")]
    assert not [n for m in others for n in m.SIGNATURES if n.startswith("kqf_")]
    assert all(n.startswith("kqf_") for n in X.SIGNATURES)
    pkg = load_pkg()
    assert pkg.IqCorrector is X.IqCorrector and "IqCorrector" in pkg.__all__ and pkg.imbalance_of is X.imbalance_of
    for name in ("blocks_dev", "accumulate_dev", "apply", "solve", "set_coeffs", "get_coeffs", "read_stats", "clear_stats",
                 "stats_view", "out_view", "kernel_info", "set_stream", "synchronize", "close"):
        assert callable(getattr(X.IqCorrector, name)), name
    companion = importlib.import_module("prgs-sdr-kspecanal_amd._companion")
    assert issubclass(X.IqCorrector, companion.Companion) and isinstance(X._bind, companion.Binding)
    assert X.LIB_PATH == LIB and X.IqCorrector._info_fields[-1] == "tile"
    g, p = X.imbalance_of(-0.08799946, 0.8944856)
    assert (g, p) == qm.imbalance_of(-0.08799946, 0.8944856)


def test_library_loads_without_a_gpu_and_every_refusal_before_a_device_has_its_own_text(X):
    lib = X.load()
    assert lib.kqf_abi_version() == X.ABI_VERSION
    try:
        import torch
        have_gpu = torch.cuda.is_available()
    except ImportError:
        have_gpu = False
    if not have_gpu:
        with pytest.raises(X.KsaError):
            X.IqCorrector()
    missing = os.path.join(PKG_DIR, "no_such_libksa_iqfix.so")
    with pytest.raises(X.KsaError) as e:
        X.load(missing)
    assert str(e.value) == ("libksa_iqfix.so is missing at %s -- build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950); "
                            "there is no CPU fallback" % missing)
    with pytest.raises(X.KsaError, match=r"unknown fmt \[f16\]"):
        X.IqCorrector(fmt="f16")
    ok = dict(device=0, fmt=0, u8_offset=127.5, u8_scale=127.5, max_in=64)
    texts = []
    for change, text in ((dict(fmt=4), "unknown sample format 4"), (dict(fmt=-1), "unknown sample format -1"),
                         (dict(max_in=0), "max_in 0 outside"), (dict(max_in=2 ** 28), "max_in 268435456 outside"),
                         (dict(fmt=1, u8_scale=0.0), "u8_scale 0"), (dict(fmt=1, u8_scale=np.inf), "u8_scale inf"),
                         (dict(fmt=1, u8_scale=np.nan), "u8_scale nan"), (dict(fmt=1, u8_offset=np.nan), "u8_offset nan"),
                         (dict(fmt=1, u8_offset=-np.inf), "u8_offset -inf"), (dict(device=-1), "device -1")):
        h = C.c_void_p(1)
        assert lib.kqf_create(*dict(ok, **change).values(), C.byref(h)) != 0 and h.value is None, text
        got = lib.kqf_last_error().decode()
        assert text in got, (text, got)
        texts.append(re.sub(r"-?(inf|nan|[0-9][0-9.e+-]*)", "#", got))
    assert len(set(texts)) == 5, sorted(set(texts))                # format / max_in / u8_scale / u8_offset / device
    assert lib.kqf_create(*ok.values(), None) != 0 and "null out pointer" in lib.kqf_last_error().decode()
    co, sums, p = X.Coeffs(), (C.c_int64 * 6)(), C.c_void_p()
    calls = (lambda: lib.kqf_set_stream(None, None), lambda: lib.kqf_synchronize(None),
             lambda: lib.kqf_blocks_dev(None, None, 0, 0, 0, None, 0, 0), lambda: lib.kqf_accumulate_dev(None, None, 0, 0, 0),
             lambda: lib.kqf_apply(None, None, 0, None, 0), lambda: lib.kqf_solve(None, 3, C.byref(co)),
             lambda: lib.kqf_set_coeffs(None, 0.0, 0.0, 0.0, 1.0), lambda: lib.kqf_get_coeffs(None, C.byref(co)),
             lambda: lib.kqf_read_stats(None, sums), lambda: lib.kqf_stats_dev(None, C.byref(p)), lambda: lib.kqf_clear_stats(None),
             lambda: lib.kqf_out_dev(None, C.byref(p)), lambda: lib.kqf_kernel_info(None, None, None, None, None, None))
    for call in calls:
        assert call() != 0 and lib.kqf_last_error().decode() == "null corrector object"
    lib.kqf_destroy(None)
    assert len(X.SIGNATURES) == len(calls) + 4                     # those, abi_version, last_error, create, destroy


def _body(text, name):
    """The text of the function `name` of kqf_api.hip, from its name to the closing brace in column 0."""
    start = re.search(r"^(?:int|kqf_coeffs) %s\(" % name, text, re.M).start()
    return text[start:text.index("\n}\n", start)]


def test_per_call_refusals_stand_before_the_first_hip_call():
    text = open(os.path.join(SRC_DIR, "kqf_api.hip")).read()
    hip = re.compile(r"DeviceGuard|HIP_OK|\bhip[A-Z]\w*\(|ensure_out|grow_device|\brun\(")
    expect = {"check_blocks": ["null corrector object", "nblocks %lld must be >= 0", "block_stride %lld must be >= 0",
                               "block_len %lld must be >= 0", "exceed max_in", "null input pointer", "check_iq_aligned", "past 2^30"],
              "kqf_blocks_dev": ["check_blocks", "out_stride %lld is shorter", "output pointer is not aligned"],
              "kqf_accumulate_dev": ["check_blocks"],
              "kqf_apply": ["null corrector object", "n %lld must be >= 0", "exceeds max_in", "null input pointer", "null output pointer",
                            "past 2^30"],
              "kqf_solve": ["null corrector object", "mode %d is not"],
              "kqf_set_coeffs": ["null corrector object", "must be finite"],
              "kqf_get_coeffs": ["null corrector object", "null coefficients out pointer"],
              "kqf_read_stats": ["null corrector object", "null sums pointer"]}
    for name, marks in expect.items():
        body = _body(text, name)
        first = hip.search(body)
        end = first.start() if first else len(body)
        if name == "check_blocks":
            assert first is None, "the shared argument check makes no HIP call"
        for m in marks:
            assert m in body and body.index(m) < end, (name, m)
        assert "fail(" not in body[end:].replace("return fail(\"hipMalloc", ""), name
    assert "#pragma clang fp contract(off)" in _body(text, "solve_sums")
    assert "getenv" not in text


def test_the_shared_headers_are_included_not_copied_and_no_atomic_exists():
    assert sorted(os.listdir(SRC_DIR)) == ["kqf_api.hip", "kqf_kernels.hpp"]
    for f in ("kqf_api.hip", "kqf_kernels.hpp"):
        text = open(os.path.join(SRC_DIR, f)).read()
        assert "struct DeviceGuard" not in text and "thread_local" not in text and "unpack_s16(" not in text and "unpack_u8(" not in text
        assert "atomic" not in text.lower(), f
    assert '#include "../csrc_shared/ksa_host.hpp"' in open(os.path.join(SRC_DIR, "kqf_api.hip")).read()
    assert '#include "../csrc_shared/ksa_iq.hpp"' in open(os.path.join(SRC_DIR, "kqf_kernels.hpp")).read()


# ------------------------------------------------------------------------------------------ command line
BASE = ["zeroSpan", "fftSize", "1024", "samplingRate", "2048000"]


def test_iqfix_key_parses(K, capsys):
    d = K.handle_args({}, BASE + ["iqfix", "dc+iq"])
    assert d["iqfix.spec"] == dict(mode=3, blocks=None, track=False)
    assert "WARN" not in capsys.readouterr().out
    assert K.handle_args({}, BASE + ["IQFIX", "DC", "iqfixSave", "x.npz"])["iqfix.spec"] == dict(mode=1, blocks=None, track=False)
    assert K.handle_args({}, BASE + ["iqfix", "iq:track"])["iqfix.spec"] == dict(mode=2, blocks=None, track=True)
    assert K.handle_args({}, BASE + ["frameBatch", "4", "iqfix", "dc+iq:blocks=4"])["iqfix.spec"] == dict(mode=3, blocks=4, track=False)
    assert K.handle_args({}, BASE + ["frameBatch", "4", "iqfix", "Dc+Iq:Blocks=1"])["iqfix.spec"] == dict(mode=3, blocks=1, track=False)
    d = K.handle_args({}, BASE + ["iqfix", "dc+iq:track", "zoom", "4", "density", "64:-120:0", "detect", "8:2:10", "iqFormat", "s16"])
    assert d["iqfix.spec"]["track"] and d["zoom.spec"] is not None                   # beside zoom, density and detect
    d = K.handle_args({}, BASE)
    assert d["iqfix"] == "" and d["iqfixSave"] == "" and d["iqfix.spec"] is None
    capsys.readouterr()
    d = K.handle_args({}, BASE + ["iqfixSave", "x.npz"])
    assert d["iqfix.spec"] is None and "WARN:handle_args: iqfixSave [x.npz] is ignored without iqfix" in capsys.readouterr().out


@pytest.mark.parametrize("text", ["dc+", "iq+dc", "on", ":track", "dc:", "dc:track:track", "dc:blocks=1:blocks=1", "dc:blocks=0",
                                  "dc:blocks=5", "dc:blocks", "dc:blocks=x", "dc:blocks=1.5", "dc:track=1", "dc:blocks=1:track",
                                  "dc:track:blocks=2", "dc:every"])
def test_iqfix_key_refuses_with_the_rule(K, text, capsys):
    d = {}
    with pytest.raises(SystemExit):
        K.handle_args(d, BASE + ["frameBatch", "4", "iqfix", text])
    assert d["cmd.stop"] is True
    assert K.IQFIX_RULE in capsys.readouterr().out


def test_iqfix_key_refuses_modes_and_raw_readers_each_with_its_own_text(K, tmp_path, capsys):
    for mode in (["scan", "startFreq", "100e6", "endFreq", "104.8e6"], ["fmScan"], ["quickFullScan"], ["zeroSpanSave"]):
        with pytest.raises(SystemExit):
            K.handle_args({}, mode + ["iqfix", "dc"])
        assert "iqfix [dc] is zeroSpan only" in capsys.readouterr().out
    d = K.handle_args({}, ["zeroSpanPlay", "fftSize", "512", "iqfix", "dc"])
    assert d["iqfix.spec"] is None and "WARN:handle_args: iqfix [dc] is ignored when playing saved spectra" in capsys.readouterr().out
    one = str(tmp_path / "one.npy")
    np.save(one, np.ones(8, dtype=np.complex64))
    for other, name, value in ((["channels", "8"], "channels", "8"), (["correlate", one], "correlate", one),
                               (["pulses", "-10:-20"], "pulses", "-10:-20")):
        with pytest.raises(SystemExit):
            K.handle_args({}, BASE + other + ["iqfix", "dc"])
        assert "iqfix [dc] corrects the blocks the engine and zoom read: %s [%s] reads the raw blocks" % (name, value) in capsys.readouterr().out
    with pytest.raises(SystemExit):
        K.handle_args({}, BASE + ["bUsePSD", "true", "iqfix", "dc"])
    assert "iqfix [dc] needs bUsePSD false" in capsys.readouterr().out
    with pytest.raises(SystemExit):                                  # fullSize is 1048576 here: 256 of them are 2^28
        K.handle_args({}, ["zeroSpan", "fftSize", "1048576", "samplingRate", "1048576", "frameBatch", "256", "iqfix", "dc"])
    out = capsys.readouterr().out
    assert "iqfix [dc]: frameBatch [256] x [" in out and "exceed the corrector's [268435455] per call" in out
