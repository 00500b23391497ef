"""Host side of the pulse detector (no GPU needed): the companion header and library, the binding, the model
every GPU test compares against on hand-worked cases, and the `pulses` / `pulsesSave` keys of the command line."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import pulse_model as pm
from companion_helper import BY_MODULE, check_header_exports_binding
from conftest import ROOT, load_pkg

PKG_DIR = os.path.join(ROOT, "prgs-sdr-kspecanal_amd")
LIB = os.path.join(PKG_DIR, "libksa_pulse.so")
OFFSETS = {"start": 0, "len": 8, "energy": 16, "peak": 24, "peak_pos": 32, "dre": 40, "dim": 48, "block": 56, "flags": 60}


@pytest.fixture(scope="module")
def X():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.pulse")


@pytest.fixture(scope="module")
def K():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")


# ------------------------------------------------------------------------------------------ header, exports, binding
def test_header_is_c99_and_matches_the_exports_and_the_binding(X, tmp_path):
    extra = ('typedef kpl_detector* handle;\ntypedef char record_is_64_bytes[sizeof(kpl_pulse) == 64 ? 1 : -1];\n'
             + "".join('typedef char %s_at_%d[offsetof(kpl_pulse, %s) == %d ? 1 : -1];\n' % (f, o, f, o) for f, o in OFFSETS.items()))
    text, _ = check_header_exports_binding(BY_MODULE["pulse"], X, tmp_path, extra,
                                           ["KPL_MAX_W", "KPL_FMT_S16", "(int)(KPL_MAX_POSITION >> 40)", "KPL_FLAG_OPEN_END"])
    assert X.ABI_VERSION == 1
    for name, value in (("KPL_MAX_W", X.MAX_W), ("KPL_MAX_MIN_LEN", X.MAX_MIN_LEN), ("KPL_MAX_CAPACITY", X.MAX_CAPACITY),
                        ("KPL_MAX_IN", X.MAX_IN), ("KPL_MAX_POSITION", X.MAX_POSITION), ("KPL_POWER_UNIT", X.POWER_UNIT),
                        ("KPL_FLAG_OPEN_END", X.FLAG_OPEN_END), ("KPL_FMT_C64", X.FMT_C64), ("KPL_FMT_U8", X.FMT_U8),
                        ("KPL_FMT_S8", X.FMT_S8), ("KPL_FMT_S16", X.FMT_S16)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value, name
    assert X.MAX_W == 4096 and X.MAX_IN == 2 ** 28 - 1 and X.MAX_POSITION == 2 ** 52 and X.POWER_UNIT == 2 ** 30 == pm.UNIT
    assert X.MAX_MIN_LEN == X.MAX_CAPACITY == 2 ** 20 and X.FLAG_OPEN_END == pm.FLAG_OPEN_END == 1
    ddc = importlib.import_module("prgs-sdr-kspecanal_amd.ddc")
    assert (X.FMT_C64, X.FMT_U8, X.FMT_S8, X.FMT_S16) == (ddc.FMT_C64, ddc.FMT_U8, ddc.FMT_S8, ddc.FMT_S16) == (0, 1, 2, 3)
    # the record: the binding's dtype, the model's and the header's struct are one layout
    assert X.EVENT_DTYPE == pm.EVENT_DTYPE and X.EVENT_DTYPE.itemsize == 64
    assert {n: X.EVENT_DTYPE.fields[n][1] for n in X.EVENT_DTYPE.names} == OFFSETS
    fields = re.search(r"typedef struct kpl_pulse \{(.*?)\} kpl_pulse;", text, re.S).group(1)
    assert re.findall(r"(?:int64_t|int32_t)\s+(\w+);", fields) == list(X.EVENT_DTYPE.names)


def test_the_other_bindings_hold_no_kpl_name_and_the_package_exports_the_class(X):
    others = [importlib.import_module("prgs-sdr-kspecanal_amd." + m)
              for m in ("_lib", "density", "mask", "ddc", "detect", "demod", "chan", "resamp", "corr")]
    assert not [n for m in others for n in m.SIGNATURES if n.startswith("kpl_")]
    assert all(n.startswith("kpl_") for n in X.SIGNATURES)
    pkg = load_pkg()
    assert pkg.PulseDetector is X.PulseDetector and "PulseDetector" in pkg.__all__
    assert pkg.PULSE_DTYPE is X.EVENT_DTYPE and (pkg.FLAG_OPEN_END, pkg.POWER_UNIT) == (1, 2 ** 30)
    assert {"PULSE_DTYPE", "FLAG_OPEN_END", "POWER_UNIT"} <= set(pkg.__all__)
    for name in ("process_dev", "process", "flush", "blocks_dev", "set_params", "thresholds", "reset", "state", "events",
                 "clear_events", "events_view", "kernel_info", "set_stream", "synchronize", "close"):
        assert callable(getattr(X.PulseDetector, name)), name
    companion = importlib.import_module("prgs-sdr-kspecanal_amd._companion")
    engine = importlib.import_module("prgs-sdr-kspecanal_amd.engine")
    assert issubclass(X.PulseDetector, companion.Companion) and isinstance(X._bind, companion.Binding) and X.DevArray is engine.DevArray
    assert X.KsaError is importlib.import_module("prgs-sdr-kspecanal_amd._lib").KsaError
    assert X.LIB_PATH == LIB and callable(X.load) and callable(X.lib) and callable(X.check)
    assert X.PulseDetector._info_fields[-1] == "tile"


def test_library_loads_without_a_gpu_and_every_create_time_refusal_has_its_own_text(X):
    lib = X.load()
    assert lib.kpl_abi_version() == X.ABI_VERSION
    try:
        import torch
        have_gpu = torch.cuda.is_available()
    except ImportError:
        have_gpu = False
    if not have_gpu:
        with pytest.raises(X.KsaError):
            X.PulseDetector()
    missing = os.path.join(PKG_DIR, "no_such_libksa_pulse.so")
    with pytest.raises(X.KsaError) as e:
        X.load(missing)
    assert str(e.value) == ("libksa_pulse.so is missing at %s -- build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950); "
                            "there is no CPU fallback" % missing)
    with pytest.raises(X.KsaError, match=r"unknown fmt \[f16\]"):              # the binding's own refusal comes before the library
        X.PulseDetector(fmt="f16")
    texts = []
    # (device, fmt, u8_offset, u8_scale, W, on_power, off_power, min_len, capacity, max_in)
    ok = (0, 0, 127.5, 127.5, 16, 0.5, 0.25, 1, 16, 64)

    def with_(**kw):
        names = ("device", "fmt", "u8_offset", "u8_scale", "W", "on_power", "off_power", "min_len", "capacity", "max_in")
        return tuple(kw.get(n, v) for n, v in zip(names, ok))

    for args, text in ((with_(fmt=4), "unknown sample format 4"), (with_(fmt=-1), "unknown sample format -1"),
                       (with_(W=0), "W 0 outside"), (with_(W=4097), "W 4097 outside"),
                       (with_(on_power=0.0), "on_power 0"), (with_(on_power=4.5), "on_power 4.5"),
                       (with_(on_power=np.nan), "on_power nan"), (with_(on_power=-1.0), "on_power -1"),
                       (with_(on_power=np.inf), "on_power inf"),
                       (with_(off_power=0.0), "off_power 0"), (with_(off_power=0.75), "off_power 0.75"),
                       (with_(off_power=np.nan), "off_power nan"), (with_(off_power=-0.5), "off_power -0.5"),
                       (with_(W=1, off_power=1e-12), "gives thr_off 0 below 1"),
                       (with_(min_len=0), "min_len 0 outside"), (with_(min_len=2 ** 20 + 1), "min_len 1048577 outside"),
                       (with_(capacity=0), "pulse capacity 0 outside"), (with_(capacity=2 ** 20 + 1), "pulse capacity 1048577 outside"),
                       (with_(max_in=0), "max_in 0 outside"), (with_(max_in=2 ** 28), "max_in 268435456 outside"),
                       (with_(fmt=1, u8_scale=0.0), "u8_scale 0"), (with_(fmt=1, u8_scale=np.inf), "u8_scale inf"),
                       (with_(fmt=1, u8_offset=np.nan), "u8_offset nan"),
                       (with_(device=-1), "device -1")):
        h = C.c_void_p(1)
        assert lib.kpl_create(*args, C.byref(h)) != 0 and h.value is None, text
        got = lib.kpl_last_error().decode()
        assert text in got, (text, got)
        texts.append(re.sub(r"-?(inf|nan|[0-9][0-9.e+-]*)", "#", got))
    # format / W / on_power / off_power / thr_off / min_len / capacity / max_in / u8_scale / u8_offset / device
    assert len(set(texts)) == 11, sorted(set(texts))
    h = C.c_void_p(1)
    assert lib.kpl_create(*ok, None) != 0 and "null out pointer" in lib.kpl_last_error().decode()
    if not have_gpu:                                    # the u8 values are only read for KPL_FMT_U8; only a device is missing then
        assert lib.kpl_create(*with_(u8_scale=0.0), C.byref(h)) != 0 and h.value is None
        assert "hip" in lib.kpl_last_error().decode()
    # a null object is refused by every entry point that takes one
    calls = (lambda: lib.kpl_set_stream(None, None), lambda: lib.kpl_synchronize(None),
             lambda: lib.kpl_process_dev(None, None, 0, None), lambda: lib.kpl_process(None, None, 0, None),
             lambda: lib.kpl_flush(None), lambda: lib.kpl_blocks_dev(None, None, 0, 0, 0, None, 0),
             lambda: lib.kpl_set_params(None, 0.5, 0.25), lambda: lib.kpl_thresholds(None, None, None), lambda: lib.kpl_reset(None),
             lambda: lib.kpl_state(None, None, None, None), lambda: lib.kpl_read_events(None, None, 0, None, None, None),
             lambda: lib.kpl_events_dev(None, None, None), lambda: lib.kpl_clear_events(None),
             lambda: lib.kpl_kernel_info(None, None, None, None, None, None))
    for call in calls:
        assert call() != 0 and "null detector object" in lib.kpl_last_error().decode()
    lib.kpl_destroy(None)
    assert len(X.SIGNATURES) == len(calls) + 4          # those, abi_version, last_error, create, destroy


def test_the_pulse_sources_hold_no_atomic():
    for f in ("kpl_api.hip", "kpl_kernels.hpp"):
        text = open(os.path.join(PKG_DIR, "csrc_pulse", f)).read()
        assert "atomic" not in text.replace("no atomic is involved", "")


# ------------------------------------------------------------------------------------------ the model on hand-worked cases
def test_hysteresis_at_the_exact_levels():
    on, off = 100, 40
    S = np.array([0, 99, 100, 50, 40, 39, 40, 99, 100, 100, 0], dtype=np.int64)
    #             -   -   SET  hold hold CLR hold hold SET  SET  CLR
    assert list(pm.active_of(S, on, off)) == [False, False, True, True, True, False, False, False, True, True, False]
    assert list(pm.active_of(np.array([40, 41, 99], dtype=np.int64), on, off)) == [False] * 3      # HOLD before any SET is inactive
    # on_power equal to off_power: no HOLD exists, active is S >= thr
    S = np.array([9, 10, 11, 10, 9, 10], dtype=np.int64)
    assert list(pm.active_of(S, 10, 10)) == [False, True, True, True, False, True]
    assert pm.thresholds(0.25, 0.0625, 1) == (2 ** 28, 2 ** 26) and pm.thresholds(4.0, 4.0, 4096) == (2 ** 44, 2 ** 44)
    assert pm.thresholds(0.1, 0.1, 3) == (int(np.rint(float(np.float32(0.1)) * 2 ** 30 * 3)),) * 2


def test_quantities_envelope_and_records_by_hand():
    # amplitudes whose powers are exact: 0.5 -> q = 2^28, 0.25 -> 2^26, 3 -> |x|^2 = 9 saturates at 4 -> 2^32
    x = np.array([0, 0.5, 0.5j, 0.25, 0, 3, 0], dtype=np.complex64)
    q, dre, dim = pm.quantities(x.real, x.imag)
    assert list(q) == [0, 2 ** 28, 2 ** 28, 2 ** 26, 0, 2 ** 32, 0]
    # x[2] conj(x[1]) = 0.25j, x[3] conj(x[2]) = -0.125j
    assert (dre[2], dim[2], dre[3], dim[3]) == (0, 2 ** 28, 0, -2 ** 27)
    assert list(pm.envelope(q, 1)) == list(q)
    assert list(pm.envelope(q, 2)) == [0, 2 ** 28, 2 ** 29, 2 ** 28 + 2 ** 26, 2 ** 26, 2 ** 32, 2 ** 32]
    assert list(pm.envelope(q, 100)) == list(np.cumsum(q))
    # W = 1, on at 0.25 (S exactly thr_on is SET), off at 0.0625 (S exactly thr_off is HOLD)
    S, ev, act = pm.detect(x, 1, 0.25, 0.0625)
    assert list(act) == [False, True, True, True, False, True, False]
    assert [tuple(e) for e in ev] == [(1, 3, 2 ** 29 + 2 ** 26, 2 ** 28, 1, 0, 2 ** 28 - 2 ** 27, -1, 0), (5, 1, 2 ** 32, 2 ** 32, 5, 0, 0, -1, 0)]
    assert len(pm.detect(x, 1, 0.25, 0.0625, min_len=2)[1]) == 1 and len(pm.detect(x, 1, 0.25, 0.0625, min_len=4)[1]) == 0
    # a run still active at the end: listed with the flag when flushed (and in a block), not at all before
    S, ev, act = pm.detect(x[:4], 1, 0.25, 0.0625, block=7)
    assert [tuple(e) for e in ev] == [(1, 3, 2 ** 29 + 2 ** 26, 2 ** 28, 1, 0, 2 ** 28 - 2 ** 27, 7, pm.FLAG_OPEN_END)]
    assert len(pm.detect(x[:4], 1, 0.25, 0.0625, flushed=False)[1]) == 0
    # the integer formats give q exactly
    s16 = np.array([[16384, 0], [0, -32768], [1, 1]], dtype=np.int16)
    assert list(pm.quantities(*pm.unpack(s16, "s16"))[0]) == [2 ** 28, 2 ** 30, 2]
    s8 = np.array([[64, 0], [-128, -128]], dtype=np.int8)
    assert list(pm.quantities(*pm.unpack(s8, "s8"))[0]) == [2 ** 28, 2 ** 31]
    u8 = np.array([[255, 0]], dtype=np.uint8)
    assert list(pm.quantities(*pm.unpack(u8, "u8"))[0]) == [2 ** 31]
    d = pm.describe(ev, 1, 1000.0, 100)
    assert d["toa_s"][0] == 0.701 and d["width_s"][0] == 0.003 and abs(d["freq_hz"][0] - 250.0) < 1e-9
    assert abs(d["peak_dbfs"][0] - 10 * np.log10(0.25)) < 1e-12


def test_describe_matches_the_model(X):
    x = np.array([0, 0.5, 0.5j, 0.25, 0, 3, 0], dtype=np.complex64)
    ev = pm.detect(x, 1, 0.25, 0.0625, block=2)[1]
    got, want = X.describe(ev, 1, 48000.0, 4096), pm.describe(ev, 1, 48000.0, 4096)
    assert sorted(got) == sorted(want) == ["freq_hz", "mean_dbfs", "peak_dbfs", "toa_s", "width_s"]
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert X.db_to_power(0) == 1.0 and X.db_to_power(-10) == float(np.float32(0.1))


# ------------------------------------------------------------------------------------------ command line
BASE = ["zeroSpan", "fftSize", "1024", "samplingRate", "2048000"]


def test_pulses_key_parses(K, capsys):
    d = K.handle_args({}, BASE + ["pulses", "-10:-20"])
    s = d["pulse.spec"]
    assert s == dict(rel=False, on_db=-10.0, off_db=-20.0, W=16, min_len=1, capacity=1024)
    assert "WARN" not in capsys.readouterr().out
    s = K.handle_args({}, BASE + ["PULSES", "rel:12:6:64:5:events=7", "pulsesSave", "x.npz"])["pulse.spec"]
    assert s == dict(rel=True, on_db=12.0, off_db=6.0, W=64, min_len=5, capacity=7)
    s = K.handle_args({}, BASE + ["pulses", "REL:40:40:4096"])["pulse.spec"]         # rel: levels above 6 dB are fine
    assert s == dict(rel=True, on_db=40.0, off_db=40.0, W=4096, min_len=1, capacity=1024)
    s = K.handle_args({}, BASE + ["pulses", "6:-3.5:1:1048576"])["pulse.spec"]
    assert (s["on_db"], s["off_db"], s["W"], s["min_len"]) == (6.0, -3.5, 1, 2 ** 20)
    d = K.handle_args({}, BASE)
    assert d["pulses"] == "" and d["pulsesSave"] == "" and d["pulse.spec"] is None
    capsys.readouterr()
    d = K.handle_args({}, BASE + ["pulsesSave", "x.npz"])
    assert d["pulse.spec"] is None and "WARN:handle_args: pulsesSave [x.npz] is ignored without pulses" in capsys.readouterr().out


@pytest.mark.parametrize("text", ["-10", "-10:", ":-20", "-20:-10", "x:-20", "-10:nan", "inf:-10", "7:0", "-10:-20:0", "-10:-20:4097",
                                  "-10:-20:2.5", "-10:-20:16:0", "-10:-20:16:1048577", "-10:-20:16:x", "-10:-20:16:1:events=0",
                                  "-10:-20:16:1:events=1048577", "-10:-20:16:1:events", "-10:-20:16:1:capacity=3",
                                  "-10:-20:16:1:events=3:1", "rel", "rel:5", "rel:5:6", "abs:-10:-20", "-10:-200:1"])
def test_pulses_key_refuses_with_the_rule(K, text, capsys):
    d = {}
    with pytest.raises(SystemExit):
        K.handle_args(d, BASE + ["pulses", text])
    assert d["cmd.stop"] is True
    assert K.PULSE_RULE in capsys.readouterr().out


def test_pulses_key_refuses_modes_and_front_ends_each_with_its_own_text(K, tmp_path, capsys):
    for mode in (["scan", "startFreq", "100e6", "endFreq", "104.8e6"], ["fmScan"], ["quickFullScan"], ["zeroSpanSave"]):
        with pytest.raises(SystemExit):
            K.handle_args({}, mode + ["pulses", "-10:-20"])
        assert "pulses [-10:-20] is zeroSpan only" in capsys.readouterr().out
    d = K.handle_args({}, ["zeroSpanPlay", "fftSize", "512", "pulses", "-10:-20"])
    assert d["pulse.spec"] is None and "pulses [-10:-20] is ignored when playing saved spectra" in capsys.readouterr().out
    for front, name in ((["zoom", "8"], "zoom"), (["channels", "8"], "channels")):
        with pytest.raises(SystemExit):
            K.handle_args({}, BASE + front + ["pulses", "-10:-20"])
        out = capsys.readouterr().out
        assert "pulses [-10:-20] reads the raw blocks: detecting pulses behind zoom or channels is out of scope, drop [%s]" % name in out
    one = str(tmp_path / "one.npy")
    np.save(one, np.ones(8, dtype=np.complex64))
    d = K.handle_args({}, BASE + ["correlate", one, "pulses", "-10:-20"])            # allowed beside correlate
    assert d["corr.spec"] is not None and d["pulse.spec"] is not None
