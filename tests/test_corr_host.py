"""Host side of the correlator (no GPU needed): the companion header and library, the binding, the model every
GPU test compares against, the helpers, and the `correlate` / `correlateSave` keys of the command line."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import corr_model as cm
from companion_helper import BY_MODULE, check_header_exports_binding
from conftest import ROOT, load_pkg

PKG_DIR = os.path.join(ROOT, "prgs-sdr-kspecanal_amd")
LIB = os.path.join(PKG_DIR, "libksa_corr.so")


@pytest.fixture(scope="module")
def X():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.corr")


@pytest.fixture(scope="module")
def K():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")


# ------------------------------------------------------------------------------------------ header, exports, binding
def test_header_is_c99_and_matches_the_exports_and_the_binding(X, tmp_path):
    extra = ('typedef kcr_corr* handle;\ntypedef char event_is_36_bytes[sizeof(kcr_event) == 36 ? 1 : -1];\n'
             'typedef char block_at_8[offsetof(kcr_event, block) == 8 && offsetof(kcr_event, im) == 32 ? 1 : -1];\n')
    text, _ = check_header_exports_binding(BY_MODULE["corr"], X, tmp_path, extra,
                                           ["KCR_MAX_K", "KCR_FMT_S16", "(int)(KCR_MAX_POSITION >> 40)"])
    for name, value in (("KCR_MAX_K", X.MAX_K), ("KCR_MAX_Q", X.MAX_Q), ("KCR_MAX_TEMPLATE_VALUES", X.MAX_TEMPLATE_VALUES),
                        ("KCR_MAX_GUARD", X.MAX_GUARD), ("KCR_MAX_CAPACITY", X.MAX_CAPACITY), ("KCR_MAX_IN", X.MAX_IN),
                        ("KCR_MAX_POSITION", X.MAX_POSITION), ("KCR_FMT_C64", X.FMT_C64), ("KCR_FMT_U8", X.FMT_U8),
                        ("KCR_FMT_S8", X.FMT_S8), ("KCR_FMT_S16", X.FMT_S16)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value, name
    assert X.MAX_IN == 2 ** 28 - 1 and X.MAX_POSITION == 2 ** 52
    ddc = importlib.import_module("prgs-sdr-kspecanal_amd.ddc")
    assert (X.FMT_C64, X.FMT_U8, X.FMT_S8, X.FMT_S16) == (ddc.FMT_C64, ddc.FMT_U8, ddc.FMT_S8, ddc.FMT_S16) == (0, 1, 2, 3)
    # the record: the binding's dtype, the model's and the header's struct are one layout
    assert X.EVENT_DTYPE == cm.EVENT_DTYPE and X.EVENT_DTYPE.itemsize == 36
    fields = re.search(r"typedef struct kcr_event \{(.*?)\} kcr_event;", text, re.S).group(1)
    assert re.findall(r"(?:int64_t|int32_t|float)\s+(\w+);", fields) == list(X.EVENT_DTYPE.names)


def test_the_other_bindings_hold_no_kcr_name_and_the_package_exports_the_class(X):
    others = [importlib.import_module("prgs-sdr-kspecanal_amd." + m)
              for m in ("_lib", "density", "mask", "ddc", "detect", "demod", "chan", "resamp")]
    assert not [n for m in others for n in m.SIGNATURES if n.startswith("kcr_")]
    assert all(n.startswith("kcr_") for n in X.SIGNATURES)
    pkg = load_pkg()
    for name in ("Correlator", "frequency_bank", "refine"):
        assert getattr(pkg, name) is getattr(X, name) and name in pkg.__all__
    for name in ("process_dev", "process", "out_count", "flush", "blocks_dev", "set_params", "set_templates", "reset", "state",
                 "events", "clear_events", "kernel_info", "set_stream", "synchronize", "close"):
        assert callable(getattr(X.Correlator, name)), name
    companion = importlib.import_module("prgs-sdr-kspecanal_amd._companion")
    engine = importlib.import_module("prgs-sdr-kspecanal_amd.engine")
    assert issubclass(X.Correlator, companion.Companion) and isinstance(X._bind, companion.Binding) and X.DevArray is engine.DevArray
    assert X.KsaError is importlib.import_module("prgs-sdr-kspecanal_amd._lib").KsaError
    assert X.LIB_PATH == LIB and callable(X.load) and callable(X.lib) and callable(X.check)


def test_library_loads_without_a_gpu_and_every_create_time_refusal_has_its_own_text(X):
    lib = X.load()
    assert lib.kcr_abi_version() == X.ABI_VERSION
    try:
        import torch
        have_gpu = torch.cuda.is_available()
    except ImportError:
        have_gpu = False
    if not have_gpu:
        with pytest.raises(X.KsaError):
            X.Correlator(np.ones(8, dtype=np.complex64))
    missing = os.path.join(PKG_DIR, "no_such_libksa_corr.so")
    with pytest.raises(X.KsaError) as e:
        X.load(missing)
    assert str(e.value) == ("libksa_corr.so is missing at %s -- build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950); "
                            "there is no CPU fallback" % missing)
    with pytest.raises(X.KsaError, match=r"unknown fmt \[f16\]"):              # the binding's own refusals come before the library
        X.Correlator(np.ones(8, dtype=np.complex64), fmt="f16")
    with pytest.raises(X.KsaError, match="templates want complex"):
        X.Correlator(np.ones((2, 2, 2), dtype=np.complex64))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    t = np.ones((2, 8, 2), dtype=np.float32)
    nan, inf, zero = t.copy(), t.copy(), t.copy()
    nan[1, 3, 0], inf[0, 5, 1], zero[1] = np.nan, np.inf, 0
    big = np.ones((8, 4096, 2), dtype=np.float32)
    texts = []
    # (device, fmt, u8_offset, u8_scale, K, Q, templates, threshold, min_energy, guard, capacity, max_in)
    ok = (0, 0, 127.5, 127.5, 8, 2, p(t), 0.5, 0.0, 4, 16, 64)

    def with_(**kw):
        names = ("device", "fmt", "u8_offset", "u8_scale", "K", "Q", "templates", "threshold", "min_energy", "guard", "capacity", "max_in")
        return tuple(kw.get(n, v) for n, v in zip(names, ok))

    for args, text in ((with_(fmt=4), "unknown sample format 4"), (with_(fmt=-1), "unknown sample format -1"),
                       (with_(K=0), "K 0 outside"), (with_(K=4097, templates=p(big)), "K 4097 outside"),
                       (with_(Q=0), "Q 0 outside"), (with_(Q=9, templates=p(big)), "Q 9 outside"),
                       (with_(K=4096, Q=5, templates=p(big)), "20480 template values exceed 16384"),
                       (with_(templates=None), "null templates"),
                       (with_(templates=p(nan)), "template 1 has a non-finite value at index 3"),
                       (with_(templates=p(inf)), "template 0 has a non-finite value at index 5"),
                       (with_(templates=p(zero)), "template 1 has zero energy"),
                       (with_(threshold=0.0), "threshold 0"), (with_(threshold=1.5), "threshold 1.5"),
                       (with_(threshold=np.nan), "threshold nan"), (with_(threshold=-0.5), "threshold -0.5"),
                       (with_(min_energy=-1.0), "min_energy -1"), (with_(min_energy=np.inf), "min_energy inf"),
                       (with_(min_energy=np.nan), "min_energy nan"),
                       (with_(guard=0), "guard 0 outside"), (with_(guard=4097), "guard 4097 outside"),
                       (with_(capacity=0), "event capacity 0 outside"), (with_(capacity=2 ** 20 + 1), "event capacity 1048577 outside"),
                       (with_(max_in=0), "max_in 0 outside"), (with_(max_in=2 ** 28), "max_in 268435456 outside"),
                       (with_(fmt=1, u8_scale=0.0), "u8_scale 0"), (with_(fmt=1, u8_scale=np.inf), "u8_scale inf"),
                       (with_(fmt=1, u8_offset=np.nan), "u8_offset nan"),
                       (with_(device=-1), "device -1")):
        h = C.c_void_p(1)
        assert lib.kcr_create(*args, C.byref(h)) != 0 and h.value is None, text
        got = lib.kcr_last_error().decode()
        assert text in got, (text, got)
        texts.append(re.sub(r"-?(inf|nan|[0-9][0-9.e+]*)", "#", got))
    # format / K / Q / Q K / null templates / non-finite value / zero energy / threshold / min_energy / guard / capacity /
    # max_in / u8_scale / u8_offset / device
    assert len(set(texts)) == 15, sorted(set(texts))
    h = C.c_void_p(1)
    assert lib.kcr_create(*ok, None) != 0 and "null out pointer" in lib.kcr_last_error().decode()
    if not have_gpu:                                    # the u8 values are only read for KCR_FMT_U8; only a device is missing then
        assert lib.kcr_create(*with_(u8_scale=0.0), C.byref(h)) != 0 and h.value is None
        assert "hip" in lib.kcr_last_error().decode()
    # a null object is refused by every entry point that takes one
    n = C.c_int64()
    calls = (lambda: lib.kcr_set_stream(None, None), lambda: lib.kcr_synchronize(None), lambda: lib.kcr_out_count(None, 1, C.byref(n)),
             lambda: lib.kcr_process_dev(None, None, 0, None, None, 0, None), lambda: lib.kcr_process(None, None, 0, None, None, 0, None),
             lambda: lib.kcr_flush(None), lambda: lib.kcr_blocks_dev(None, None, 0, 0, 0, None, None, 0),
             lambda: lib.kcr_set_params(None, 0.5, 0.0), lambda: lib.kcr_set_templates(None, None), lambda: lib.kcr_reset(None),
             lambda: lib.kcr_state(None, None, None, None), lambda: lib.kcr_read_events(None, None, 0, None, None),
             lambda: lib.kcr_events_dev(None, None, None), lambda: lib.kcr_clear_events(None),
             lambda: lib.kcr_kernel_info(None, None, None, None, None, None))
    for call in calls:
        assert call() != 0 and "null correlator" in lib.kcr_last_error().decode()
    lib.kcr_destroy(None)
    assert len(X.SIGNATURES) == len(calls) + 4          # those, abi_version, last_error, create, destroy


# ------------------------------------------------------------------------------------------ the model checks itself
@pytest.mark.parametrize("K_", [1, 7, 256, 4096])
def test_float32_emulation_stays_inside_the_bound(K_):
    rng = np.random.default_rng(1000 + K_)
    Q, n = (3, 40) if K_ < 4096 else (1, 24)
    c = (rng.uniform(-1, 1, (Q, K_)) + 1j * rng.uniform(-1, 1, (Q, K_))).astype(np.complex64)
    x = (rng.uniform(-1, 1, n + K_ - 1) + 1j * rng.uniform(-1, 1, n + K_ - 1)).astype(np.complex64)
    rho, r = cm.f32_chain(x, c)
    assert rho.dtype == np.float32 and r.dtype == np.complex64 and rho.shape == r.shape == (Q, n)
    w_rho, w_r = cm.worst_ratios(rho, r, x, c)
    print("correlator emulation K %d: rho error / bound %.4f, r error / bound %.4f" % (K_, w_rho, w_r))
    assert w_rho <= 1.0 and w_r <= 1.0
    want, _ = cm.definition(x, c)
    assert np.all(want <= 1 + 1e-12) and np.all(want >= 0)                      # Cauchy-Schwarz
    if K_ == 1:
        assert np.allclose(want, 1.0, rtol=0, atol=1e-12)                       # one sample is always a multiple of one tap


def test_definition_on_a_copy_of_the_template_and_counts():
    rng = np.random.default_rng(5)
    c = (rng.standard_normal(16) + 1j * rng.standard_normal(16)).astype(np.complex64)
    x = np.zeros(64, dtype=np.complex128)
    x[20:36] = (0.3 - 0.4j) * c.astype(np.complex128)
    rho, r = cm.definition(x, c)
    assert rho.shape == (1, 49) and abs(rho[0, 20] - 1) < 1e-12 and np.argmax(rho[0]) == 20
    assert np.allclose(r[0, 20], (0.3 - 0.4j) * np.sum(np.abs(c.astype(np.complex128)) ** 2))
    assert np.all(rho[0, :5] == 0) and np.all(rho[0, 36:] == 0)                 # windows of zero energy
    assert cm.definition(x[:15], c)[0].shape == (1, 0)
    assert cm.definition(x, c, min_energy=1e9)[0].max() == 0
    at, total = 0, 0
    for n in rng.integers(0, 40, 50):
        total += cm.out_count(at, int(n), 16)
        at += int(n)
    assert total == cm.lags_after(at, 16) and cm.out_count(0, 15, 16) == 0 and cm.out_count(15, 1, 16) == 1


@pytest.mark.parametrize("shape", [(1, 1), (2, 1), (7, 3), (64, 1), (255, 2), (256, 8)], ids=str)
def test_exact_generators_are_exact(shape):
    K_, Q = shape
    rng = np.random.default_rng(K_ * 31 + Q)
    c = cm.exact_templates(rng, Q, K_)
    x = cm.exact_samples(rng, K_ + 50)
    for me in (0.0, 8.0 * K_):
        rho, r = cm.exact_model(x, c, me)
        rho32, r32 = cm.f32_chain(x, c, me)
        rho64, r64 = cm.definition(x, c, me)
        assert rho.dtype == np.float32 and np.array_equal(rho, rho32) and np.array_equal(r, r32)
        assert np.array_equal(r.astype(np.complex128), r64)
        assert np.array_equal(rho, rho64.astype(np.float32))                    # one rounding: the division
    assert np.array_equal(cm.ec32(c), np.full(Q, K_, dtype=np.float32))


def test_peak_rule_on_plateaus_ties_and_edges():
    f = lambda *v: np.array(v, dtype=np.float32)
    assert cm.peaks(f(0, .6, 0, 0, .7, 0), .5, 1) == [1, 4]
    assert cm.peaks(f(0, .6, 0, 0, .7, 0), .5, 3) == [4]                       # .6 has the larger .7 three lags on
    assert cm.peaks(f(0, .6, 0, 0, .7, 0), .5, 2) == [1, 4]
    assert cm.peaks(f(0, .7, 0, 0, .6, 0), .5, 3) == [1]
    assert cm.peaks(f(.8, .8, .8, .8), .5, 1) == [0]                           # a plateau: the lowest lag among equals
    assert cm.peaks(f(.8, .8, .8, .8), .5, 4) == [0]
    assert cm.peaks(f(.8, 0, .8, 0, .8), .5, 1) == [0, 2, 4]                   # equals further apart than G are all peaks
    assert cm.peaks(f(.8, 0, .8, 0, .8), .5, 2) == [0]
    assert cm.peaks(f(.8, 0, 0, .8, 0, 0, .8), .5, 2) == [0, 3, 6]
    assert cm.peaks(f(.9, .1), .5, 5) == [0] and cm.peaks(f(.1, .9), .5, 5) == [1]      # the edges: missing lags constrain nothing
    assert cm.peaks(f(.5), .5, 1) == [0] and cm.peaks(f(.4999), .5, 1) == [] and cm.peaks(f(), .5, 1) == []
    assert cm.peaks(f(.6, .7, .8, .9), .5, 1) == [3] and cm.peaks(f(.9, .8, .7, .6), .5, 1) == [0]
    assert cm.peaks(f(.9, .8, .7, .6, .9), .5, 3) == [0, 4] and cm.peaks(f(.9, .8, .7, .6, .9), .5, 4) == [0]
    rho = np.array([f(0, .6, .5, 0, .9), f(.7, 0, 0, .7, 0)])
    r = (rho * (1 + 2j)).astype(np.complex64)
    ev = cm.records(rho, r, .5, 2, block=3, pos_base=100)
    assert [(e["pos"], e["block"], e["templ"]) for e in ev] == [(100, 3, 1), (101, 3, 0), (103, 3, 1), (104, 3, 0)]
    assert ev[0]["metric_prev"] == 0 and ev[0]["metric_next"] == 0 and ev[3]["metric_next"] == 0 and ev[3]["metric_prev"] == 0
    assert ev[1]["metric_prev"] == 0 and ev[1]["metric_next"] == np.float32(.5)
    assert ev[2]["metric"] == np.float32(.7) and ev[3]["re"] == np.float32(.9) and ev[3]["im"] == np.float32(.9) * 2
    assert len(cm.records(rho, r, .5, 2, first=1, last=4)) == 2                # only the decided lags are listed
    assert [tuple(e) for e in cm.records(rho, r, .5, 3)[["pos", "templ"]]] == [(0, 1), (4, 0)]     # .6 now sees .9, the later .7 the earlier
    both = cm.block_records(np.array([rho, rho]), np.array([r, r]), .5, 2)
    assert list(both["block"]) == [0] * 4 + [1] * 4 and list(both["pos"]) == [0, 1, 3, 4] * 2


# ------------------------------------------------------------------------------------------ the helpers
def test_frequency_bank_and_refine(X):
    t = np.exp(2j * np.pi * np.random.default_rng(3).uniform(0, 1, 32)).astype(np.complex64)
    bank = X.frequency_bank(t, [0.0, 0.01, -0.25])
    assert bank.dtype == np.complex64 and bank.shape == (3, 32) and np.array_equal(bank[0], t)
    assert np.allclose(bank[2], t * np.exp(-0.5j * np.pi * np.arange(32)), atol=1e-6)
    assert X.frequency_bank(t, 0.125).shape == (1, 32)
    for bad in (lambda: X.frequency_bank(t, [np.nan]), lambda: X.frequency_bank(t, []), lambda: X.frequency_bank([], [0.0])):
        with pytest.raises(X.KsaError):
            bad()
    ev = np.zeros(5, dtype=X.EVENT_DTYPE)
    ev["pos"] = [10, 20, 30, 40, 50]
    # a parabola 1 - (t - t0)^2 / 8 sampled at pos - 1, pos, pos + 1 with t0 = pos + 0.25; a symmetric one; a flat one; an edge
    # whose missing neighbour left 0 (still a proper parabola); and one with no curvature
    par = lambda t, t0: 1 - (t - t0) ** 2 / 8
    ev["metric_prev"] = [par(9, 10.25), .5, .7, 0, .2]
    ev["metric"] = [par(10, 10.25), .9, .7, .9, .5]
    ev["metric_next"] = [par(11, 10.25), .5, .7, .8, .8]
    got = X.refine(ev)
    assert abs(got[0] - 10.25) < 1e-6 and got[1] == 20 and got[2] == 30 and got[4] == 50
    assert 40 < got[3] <= 40.5
    assert np.allclose(got, cm.refine(ev)) and X.refine(ev[:0]).shape == (0,)


# ------------------------------------------------------------------------------------------ command line
BASE = ["zeroSpan", "fftSize", "1024", "samplingRate", "2048000"]


@pytest.fixture()
def tmpl(tmp_path):
    rng = np.random.default_rng(9)
    one = tmp_path / "one.npy"
    bank = tmp_path / "bank.npy"
    np.save(one, np.exp(2j * np.pi * rng.uniform(0, 1, 48)).astype(np.complex64))
    np.save(bank, np.exp(2j * np.pi * rng.uniform(0, 1, (3, 32))))
    return str(one), str(bank)


def test_correlate_key_parses(K, X, tmpl, capsys):
    one, bank = tmpl
    d = K.handle_args({}, BASE + ["correlate", one])
    s = d["corr.spec"]
    assert sorted(s) == ["capacity", "file", "guard", "templates", "threshold"]
    assert (s["file"], s["threshold"], s["guard"], s["capacity"]) == (one, 0.5, 48, 4096)
    assert s["templates"].dtype == np.complex64 and s["templates"].shape == (1, 48)
    assert "WARN" not in capsys.readouterr().out
    s = K.handle_args({}, BASE + ["CORRELATE", bank + ":0.75:5:events=7", "correlateSave", "x.npz"])["corr.spec"]
    assert (s["threshold"], s["guard"], s["capacity"]) == (0.75, 5, 7) and s["templates"].shape == (3, 32)
    assert s["templates"].dtype == np.complex64
    s = K.handle_args({}, BASE + ["correlate", bank + ":1"])["corr.spec"]
    assert (s["threshold"], s["guard"], s["capacity"]) == (1.0, 32, 4096)
    d = K.handle_args({}, BASE)
    assert d["correlate"] == "" and d["correlateSave"] == "" and d["corr.spec"] is None
    capsys.readouterr()
    d = K.handle_args({}, BASE + ["correlateSave", "x.npz"])
    assert d["corr.spec"] is None and "WARN:handle_args: correlateSave [x.npz] is ignored without correlate" in capsys.readouterr().out


@pytest.mark.parametrize("suffix", [":0", ":1.5", ":nan", ":x", ":-0.5", ":0.5:0", ":0.5:4097", ":0.5:x", ":0.5:2.5", ":0.5:4:events=0",
                                    ":0.5:4:events=1048577", ":0.5:4:events", ":0.5:4:capacity=3", ":0.5:4:events=3:1", ":inf"])
def test_correlate_key_refuses_with_the_rule(K, tmpl, suffix, capsys):
    d = {}
    with pytest.raises(SystemExit):
        K.handle_args(d, BASE + ["correlate", tmpl[0] + suffix])
    assert d["cmd.stop"] is True
    assert K.CORR_RULE in capsys.readouterr().out


def test_correlate_key_refuses_bad_files_modes_and_front_ends_each_with_its_own_text(K, tmpl, tmp_path, capsys):
    one, bank = tmpl
    files = {}
    for name, arr in (("real", np.ones(8, dtype=np.float32)), ("three", np.ones((2, 2, 2), dtype=np.complex64)),
                      ("scalar", np.complex64(1)), ("empty", np.zeros(0, dtype=np.complex64)), ("long", np.ones(4097, dtype=np.complex64)),
                      ("many", np.ones((9, 4), dtype=np.complex64)), ("big", np.ones((5, 4096), dtype=np.complex64)),
                      ("nan", np.array([1, np.nan], dtype=np.complex64)), ("zero", np.array([[1, 1], [0, 0]], dtype=np.complex64))):
        files[name] = str(tmp_path / (name + ".npy"))
        np.save(files[name], arr)
    files["missing"] = str(tmp_path / "missing.npy")
    for name, path in files.items():
        with pytest.raises(SystemExit):
            K.handle_args({}, BASE + ["correlate", path])
        out = capsys.readouterr().out
        assert "the file [%s] must hold %s" % (path, K.CORR_FILE_RULE) in out, name
    for mode in (["scan", "startFreq", "100e6", "endFreq", "104.8e6"], ["fmScan"], ["quickFullScan"], ["zeroSpanSave"]):
        with pytest.raises(SystemExit):
            K.handle_args({}, mode + ["correlate", one])
        assert "correlate [%s] is zeroSpan only" % one in capsys.readouterr().out
    d = K.handle_args({}, ["zeroSpanPlay", "fftSize", "512", "correlate", one])
    assert d["corr.spec"] is None and "correlate [%s] is ignored when playing saved spectra" % one in capsys.readouterr().out
    for front, name in ((["zoom", "8"], "zoom"), (["channels", "8"], "channels")):
        with pytest.raises(SystemExit):
            K.handle_args({}, BASE + front + ["correlate", one])
        out = capsys.readouterr().out
        assert "correlating behind zoom or channels is out of scope, drop [%s]" % name in out
    long = str(tmp_path / "k4096.npy")
    np.save(long, np.ones(4096, dtype=np.complex64))
    d = K.handle_args({}, ["zeroSpan", "fftSize", "64", "samplingRate", "64", "correlate", one])     # fullSize 64 >= 48
    assert d["fullSize"] >= 48 and d["corr.spec"] is not None
    capsys.readouterr()
    with pytest.raises(SystemExit):
        K.handle_args({}, ["zeroSpan", "fftSize", "64", "samplingRate", "64", "correlate", long])
    assert "is shorter than the template of [4096]" in capsys.readouterr().out
