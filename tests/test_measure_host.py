"""Host side of the band meter (no GPU needed): the companion header and library, the binding, the build table's second table,
the float64 model every GPU test compares against on hand-computed cases, the `measure` / `measureSave` keys of the command
line, and the library's own kernel catalogue."""
import contextlib
import ctypes as C
import importlib
import importlib.util
import io
import os
import re
import threading

import numpy as np
import pytest

import measure_model as mm
from companion_helper import Companion, PKG_DIR, SHARED, check_header_exports_binding
from conftest import ROOT, load_pkg
from test_kernel_catalogue_host import kernel_names

RECORD = Companion("measure", "libksa_measure.so", "kme_", "ksa_measure.h", "csrc_measure", "kme_api.hip", "kme_kernels.hpp",
                   "SpectrumMeter", False, lambda lib, h: lib.kme_create(0, 1024, 0, 0.99, 3.0, 0, h),
                   "result capacity 0 outside 1..1048576")


@pytest.fixture(scope="module")
def X():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.measure")


@pytest.fixture(scope="module")
def K():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")


# ------------------------------------------------------------------------------------------ header, exports, binding
def test_header_is_c99_and_matches_the_exports_the_binding_and_the_dtype(X, tmp_path):
    extra = ('typedef kme_meter* handle;\ntypedef char result_is_80_bytes[sizeof(kme_result) == 80 ? 1 : -1];\n'
             'typedef char span_is_16_bytes[sizeof(kme_span) == 16 ? 1 : -1];\n'
             + "".join('typedef char r_%s_at_%d[offsetof(kme_result, %s) == %d ? 1 : -1];\n' % (f, o, f, o) for f, o in mm.OFFSETS.items())
             + "".join('typedef char s_%s_at_%d[offsetof(kme_span, %s) == %d ? 1 : -1];\n' % (f, o, f, o)
                       for f, o in (("row", 0), ("bin_lo", 8), ("bin_hi", 12))))
    macros = ["KME_MAX_NBINS", "KME_MAX_CAPACITY", "KME_MAX_MARGIN", "KME_MAX_BANDS", "KME_WAVE_MAX_BINS", "KME_FLAG_MEASURED",
              "KME_FLAG_CLIPPED", "KME_FLAG_INVALID"]
    text, names = check_header_exports_binding(RECORD, X, tmp_path, extra, macros)
    assert "KME_ABI_VERSION 1" in text and X.ABI_VERSION == 1 and len(names) == 16
    for name, value in (("KME_MAX_NBINS", X.MAX_NBINS), ("KME_MAX_CAPACITY", X.MAX_CAPACITY), ("KME_MAX_MARGIN", X.MAX_MARGIN),
                        ("KME_MAX_BANDS", X.MAX_BANDS), ("KME_WAVE_MAX_BINS", X.WAVE_MAX_BINS), ("KME_FLAG_MEASURED", X.FLAG_MEASURED),
                        ("KME_FLAG_CLIPPED", X.FLAG_CLIPPED), ("KME_FLAG_INVALID", X.FLAG_INVALID)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value, name
    assert (X.MAX_NBINS, X.MAX_CAPACITY, X.MAX_MARGIN, X.MAX_BANDS) == (2 ** 24, 2 ** 20, 65536, 1024)
    assert (X.WAVE_MAX_BINS, X.FLAG_MEASURED, X.FLAG_CLIPPED, X.FLAG_INVALID) == (mm.WAVE_MAX_BINS, 1, 2, 4)
    # the record: the binding's dtype, the model's and the header's struct are one layout
    assert X.RESULT_DTYPE == mm.RESULT_DTYPE and X.RESULT_DTYPE.itemsize == 80
    assert {n: X.RESULT_DTYPE.fields[n][1] for n in X.RESULT_DTYPE.names} == mm.OFFSETS
    fields = re.search(r"typedef struct kme_result \{(.*?)\} kme_result;", text, re.S).group(1)
    assert re.findall(r"(?:int64_t|int32_t|float|double)\s+(\w+);", fields) == list(X.RESULT_DTYPE.names)
    # the span begins as the detector's record does, although no header includes the other
    detect = importlib.import_module("prgs-sdr-kspecanal_amd.detect")
    assert [(n, detect.EMISSION_DTYPE.fields[n]) for n in X.SPAN_HEAD_DTYPE.names] == [(n, X.SPAN_HEAD_DTYPE.fields[n]) for n in X.SPAN_HEAD_DTYPE.names]
    assert "#include" not in re.sub(r"/\*.*?\*/", "", text, flags=re.S).replace("#include <stdint.h>", "")
    assert "2^-53" in text and "ANY summation order" in text and "no float atomics" in text
    assert X.SpectrumMeter._info_fields == ("threads", "lds_bytes", "vgprs", "grid", "vec", "form")


def test_the_package_exports_the_meter_and_no_other_binding_holds_a_kme_name(X):
    names = ("_lib", "density", "mask", "ddc", "detect", "demod", "chan", "resamp", "corr", "pulse", "track", "iqfix")
    others = [importlib.import_module("prgs-sdr-kspecanal_amd." + m) for m in names]
    assert not [n for m in others for n in m.SIGNATURES if n.startswith("kme_")]
    assert all(n.startswith("kme_") for n in X.SIGNATURES)
    pkg = load_pkg()
    for name in ("SpectrumMeter", "RESULT_DTYPE", "result_freqs", "acpr"):
        assert getattr(pkg, name) is getattr(X, name) and name in pkg.__all__, name
    companion = importlib.import_module("prgs-sdr-kspecanal_amd._companion")
    engine = importlib.import_module("prgs-sdr-kspecanal_amd.engine")
    assert issubclass(X.SpectrumMeter, companion.Companion) and isinstance(X._bind, companion.Binding) and X.DevArray is engine.DevArray
    assert X.SpectrumMeter._binding is X._bind and X.KsaError is importlib.import_module("prgs-sdr-kspecanal_amd._lib").KsaError
    assert X.LIB_PATH == os.path.join(PKG_DIR, RECORD.so) and X.load == X._bind.load and X.lib == X._bind.lib and X.check == X._bind.check
    assert "def load(" not in open(os.path.join(PKG_DIR, "measure.py")).read()
    for name in ("measure_spans_dev", "measure_spans", "measure_detector", "set_bands", "measure_bands_dev", "measure_bands", "results",
                 "results_view", "reset", "set_params", "kernel_info", "set_stream", "synchronize", "close"):
        assert callable(getattr(X.SpectrumMeter, name)), name


def test_library_loads_without_a_gpu_and_every_refusal_has_its_own_text(X):
    lib = X.load()
    assert lib.kme_abi_version() == X.ABI_VERSION
    try:
        import torch
        have_gpu = torch.cuda.is_available()
    except ImportError:
        have_gpu = False
    if not have_gpu:
        with pytest.raises(X.KsaError):
            X.SpectrumMeter(1024)
    missing = os.path.join(PKG_DIR, "no_such_libksa_measure.so")
    with pytest.raises(X.KsaError) as e:
        X.load(missing)
    assert str(e.value) == ("libksa_measure.so is missing at %s -- build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950); "
                            "there is no CPU fallback" % missing)
    good = dict(device=0, nbins=1024, capacity=16, occupied=0.99, xdb=3.0, margin=0)
    texts = []
    for change, text in ((dict(nbins=0), "nbins 0 outside 1..16777216"), (dict(nbins=2 ** 24 + 1), "nbins 16777217 outside"),
                         (dict(capacity=0), "result capacity 0 outside 1..1048576"), (dict(capacity=2 ** 20 + 1), "result capacity 1048577"),
                         (dict(occupied=0.49), "occupied 0.49"), (dict(occupied=1.0), "occupied 1 "), (dict(occupied=float("nan")), "occupied nan"),
                         (dict(xdb=-0.5), "xdb -0.5"), (dict(xdb=100.5), "xdb 100.5"), (dict(xdb=float("nan")), "xdb nan"),
                         (dict(xdb=float("inf")), "xdb inf"), (dict(margin=-1), "margin -1 outside 0..65536"),
                         (dict(margin=65537), "margin 65537"), (dict(device=-1), "device -1 must be >= 0")):
        a = dict(good, **change)
        h = C.c_void_p(1)
        assert lib.kme_create(a["device"], a["nbins"], a["capacity"], a["occupied"], a["xdb"], a["margin"], C.byref(h)) != 0, text
        assert h.value is None, text
        got = lib.kme_last_error().decode()
        assert text in got, (text, got)
        texts.append(re.sub(r"-?[0-9.]+|nan|inf", "#", got))
    assert len(set(texts)) == 6, sorted(set(texts))            # nbins / capacity / occupied / xdb / margin / device
    assert lib.kme_create(0, 1024, 16, 0.99, 3.0, 0, None) != 0 and "null out" in lib.kme_last_error().decode()
    if not have_gpu:                            # every value at its limit is accepted; only a device is missing then
        for a in (dict(good, nbins=1, capacity=1, occupied=0.5, xdb=0.0), dict(good, nbins=2 ** 24, capacity=2 ** 20, xdb=100.0, margin=65536)):
            h = C.c_void_p(1)
            assert lib.kme_create(a["device"], a["nbins"], a["capacity"], a["occupied"], a["xdb"], a["margin"], C.byref(h)) != 0
            assert h.value is None and "hip" in lib.kme_last_error().decode()


def test_the_error_string_is_the_library_s_own_and_thread_local(X):
    lib = X.load()
    detect = importlib.import_module("prgs-sdr-kspecanal_amd.detect")
    h = C.c_void_p(1)
    assert detect.lib().kse_create(0, 1024, 0, 2, 10.0, 0, 1, 0, 16, C.byref(h)) != 0
    assert RECORD.refuse(lib, C.byref(h)) != 0 and h.value is None
    assert lib.kme_last_error().decode() == RECORD.refusal
    assert detect.lib().kse_last_error().decode() == "train 0 outside 1..1024"         # neither has overwritten the other's text
    seen = []
    t = threading.Thread(target=lambda: seen.append(lib.kme_last_error().decode()))
    t.start()
    t.join()
    assert seen == [""] and lib.kme_last_error().decode() == RECORD.refusal
    with pytest.raises(X.KsaError, match=re.escape(RECORD.refusal)):
        X.check(RECORD.refuse(lib, C.byref(C.c_void_p())))


def test_a_null_object_is_refused_by_every_entry_point(X):
    lib = X.load()
    p = C.c_void_p()
    buf = (C.c_float * 16)()
    calls = {
        "kme_set_stream": lambda: lib.kme_set_stream(None, None),
        "kme_synchronize": lambda: lib.kme_synchronize(None),
        "kme_set_params": lambda: lib.kme_set_params(None, 0.99, 3.0, 0),
        "kme_measure_spans_dev": lambda: lib.kme_measure_spans_dev(None, buf, 16, 1, 0, buf, 32, buf, 1, 0),
        "kme_measure_spans": lambda: lib.kme_measure_spans(None, buf, 1, 0, buf, 32, buf, 1, 0),
        "kme_set_bands": lambda: lib.kme_set_bands(None, None, 0),
        "kme_measure_bands_dev": lambda: lib.kme_measure_bands_dev(None, buf, 16, 1, 0, 0),
        "kme_measure_bands": lambda: lib.kme_measure_bands(None, buf, 1, 0, 0),
        "kme_read_results": lambda: lib.kme_read_results(None, buf, 0, 0),
        "kme_results_dev": lambda: lib.kme_results_dev(None, C.byref(p)),
        "kme_reset": lambda: lib.kme_reset(None),
        "kme_kernel_info": lambda: lib.kme_kernel_info(None, None, None, None, None, None, None),
    }
    assert set(calls) == set(X.SIGNATURES) - {"kme_abi_version", "kme_last_error", "kme_create", "kme_destroy"}
    for name, call in calls.items():
        assert call() != 0 and "null meter" in lib.kme_last_error().decode(), name
    lib.kme_destroy(None)


# ------------------------------------------------------------------------------------------ sources and the build table
def test_the_source_directory_holds_its_two_files_and_includes_the_shared_header():
    assert sorted(os.listdir(os.path.join(PKG_DIR, RECORD.src_dir))) == [RECORD.api, RECORD.kernels]
    api, kernels = (open(os.path.join(PKG_DIR, RECORD.src_dir, f)).read() for f in (RECORD.api, RECORD.kernels))
    for text in (api, kernels):
        assert "struct DeviceGuard" not in text and "thread_local" not in text and "getenv" not in text
        assert "atomic" not in text.replace("No atomics of any kind", "")
    assert '#include "../csrc_shared/ksa_host.hpp"' in api and "ksa_iq.hpp" not in api + kernels
    assert '#include "../../include/ksa_measure.h"' in api and "ksa_detect.h" not in api + kernels


def test_the_addons_table_is_the_one_row_and_products_is_unchanged():
    build = importlib.import_module("prgs-sdr-kspecanal_amd.build")
    real = os.path.realpath
    assert list(build.ADDONS.items()) == [("libksa_measure.so", ("csrc_measure", "kme_api.hip", "ksa_measure.h", []))]
    assert list(build.PRODUCTS) == ["libksa.so", "libksa_exp.so", "libksa_density.so", "libksa_mask.so", "libksa_ddc.so",
                                    "libksa_detect.so", "libksa_demod.so", "libksa_chan.so", "libksa_resamp.so", "libksa_corr.so",
                                    "libksa_pulse.so", "libksa_track.so", "libksa_iqfix.so"]
    assert len(build.JOBS) == 13 and not set(build.ADDONS) & set(build.PRODUCTS)
    assert not [j for j in build.JOBS if "measure" in j] and build.sources() == build._sources("libksa.so")
    assert (build.OUT, build.OUT_EXP) == tuple(build.JOBS)[:2]
    out = os.path.join(build.HERE, RECORD.so)
    deps = {real(f) for f in build._sources(RECORD.so)}
    assert {real(f) for f in SHARED} <= deps and real(os.path.join(ROOT, "include", RECORD.header)) in deps
    assert {real(os.path.join(PKG_DIR, RECORD.src_dir, f)) for f in (RECORD.api, RECORD.kernels)} <= deps
    assert build.is_stale(out) in (False, True) and os.path.exists(out)
    assert not [n for n in vars(build) if n not in ("PRODUCTS", "JOBS") and ("PRODUCTS" in n or "JOBS" in n or "TABLES" in n)]
    # build() compiles the row after JOBS, also when a caller has narrowed JOBS: nothing is stale here, so nothing is compiled
    narrowed = importlib.util.module_from_spec(importlib.util.spec_from_file_location("ksa_build_narrowed", os.path.join(PKG_DIR, "build.py")))
    narrowed.__spec__.loader.exec_module(narrowed)
    narrowed.JOBS = narrowed._jobs({"libksa_detect.so": narrowed.PRODUCTS["libksa_detect.so"]})
    seen = []
    narrowed.is_stale = lambda o=narrowed.OUT: seen.append(os.path.basename(o)) or False
    narrowed.build()
    assert seen == ["libksa_detect.so", "libksa_measure.so"]


# ------------------------------------------------------------------------------------------ the model checks itself
def test_model_flat_row_obw_starts_after_the_tail():
    # widths whose tail, (1 - beta) / 2 * W bins, lies well away from a whole number: there the edge is decidable
    for width, beta, a in ((80, 0.99, 10), (250, 0.99, 0), (1010, 0.9, 24), (66, 0.5, 3), (7, 0.99, 1)):
        row = np.full(a + width + 5, -30.0, dtype=np.float32)
        r, margin = mm.measure(row, a, a + width - 1, occupied=beta, xdb=3.0)
        tail_bins = (1.0 - float(np.float32(beta))) / 2 * width
        assert r["obw_lo"] == a + int(np.floor(tail_bins)) and r["obw_hi"] == a + width - 1 - int(np.floor(tail_bins)), (width, beta)
        assert margin >= 1e-4 and r["nvalid"] == width and r["flags"] == mm.FLAG_MEASURED
        assert (r["xdb_lo"], r["xdb_hi"], r["peak_bin"], r["peak_db"]) == (a, a + width - 1, a, np.float32(-30.0))
        assert abs(r["power"] - width * 1e-3) <= 1e-15 * width and abs(r["m1"] / r["power"] - (width - 1) / 2) < 1e-9
        assert r["power_db"] == np.float32(10 * np.log10(width * 1e-3))


def test_model_single_hot_bin_and_the_special_values():
    row = np.full(100, -90.0, dtype=np.float32)
    row[50] = 0.0
    r, margin = mm.measure(row, 0, 99)
    assert (r["obw_lo"], r["obw_hi"], r["xdb_lo"], r["xdb_hi"], r["peak_bin"]) == (50, 50, 50, 50, 50) and margin > 1e-3
    assert abs(r["m1"] / r["power"] - 50) < 1e-6 and abs(r["power"] - (1 + 99e-9)) < 1e-12
    row[10], row[11], row[12], row[13], row[14] = np.nan, -np.inf, np.inf, 700.0, -700.0
    r, _ = mm.measure(row, 0, 99, xdb=6.0)
    assert r["nvalid"] == 98 and r["flags"] == mm.FLAG_MEASURED | mm.FLAG_INVALID
    assert r["peak_bin"] == 12 and np.isposinf(r["peak_db"]) and (r["xdb_lo"], r["xdb_hi"]) == (12, 13)     # +inf and 700 both count as 500
    assert (r["obw_lo"], r["obw_hi"]) == (12, 13) and abs(r["power"] / 2e50 - 1) < 1e-12
    r, margin = mm.measure(row, 10, 11)
    assert (r["nvalid"], r["power"], r["peak_bin"], r["obw_lo"], r["obw_hi"], r["xdb_lo"], r["xdb_hi"]) == (0, 0.0, -1, -1, -1, -1, -1)
    assert np.isneginf(r["power_db"]) and np.isnan(r["peak_db"]) and r["flags"] == 5 and margin == np.inf
    tie = np.full(8, -50.0, dtype=np.float32)
    tie[2], tie[5] = -0.0, 0.0
    r, _ = mm.measure(tie, 0, 7)
    assert r["peak_bin"] == 2 and np.signbit(r["peak_db"])                    # the lowest bin among equals, its own bits
    v, xc, p = mm.powers(np.array([-600.0, 600.0, -10.0], dtype=np.float32))
    assert xc.tolist() == [-500.0, 500.0, -10.0] and p.tolist() == [1e-50, 1e50, 0.1]


def test_model_spans_clip_skip_and_keep_their_slots():
    rows = np.full((3, 32), -60.0, dtype=np.float32)
    rows[:, 16] = -20.0
    spans = np.zeros(6, dtype=[("row", "<i8"), ("bin_lo", "<i4"), ("bin_hi", "<i4")])
    spans[:] = [(9, 15, 17), (10, 1, 3), (11, 15, 17), (11, 20, 31), (12, 5, 4), (13, 15, 17)]
    out, margins = mm.measure_spans(rows, spans, 6, 8, margin=2, row_base=10)
    assert (out["flags"] & 1).tolist() == [0, 1, 1, 1, 0, 0, 0, 0] and out["flags"][[1, 3]].tolist() == [3, 3]
    assert out[["bin_lo", "bin_hi"]][1:4].tolist() == [(0, 5), (13, 19), (18, 31)] and out["row"][1:4].tolist() == [10, 11, 11]
    assert out["peak_bin"][2] == 16 and np.isinf(margins[[0, 4, 5, 6, 7]]).all()
    again, _ = mm.measure_spans(rows, spans, 6, 8, margin=2, row_base=10, first=2, before=np.zeros(8, dtype=mm.RESULT_DTYPE))
    assert (again["flags"] & 1).tolist() == [0, 0, 1, 1, 0, 0, 0, 0]
    bands, _ = mm.measure_bands(rows, [(0, 31), (16, 16)], 8, row_base=4, first_slot=1)
    assert bands["row"].tolist() == [0, 4, 4, 5, 5, 6, 6, 0] and bands["bin_hi"][1:7].tolist() == [31, 16] * 3


def test_result_freqs_and_acpr(X):
    freqs = np.fft.fftshift(np.fft.fftfreq(64, 1 / 2.4e6) + 92e6)
    step = 2.4e6 / 64
    res = np.zeros(3, dtype=X.RESULT_DTYPE)
    res["flags"], res["nvalid"] = [1, 1, 0], [5, 0, 0]
    res["bin_lo"], res["power"], res["m1"] = [10, 0, 0], [2.0, 0.0, 0.0], [3.0, 0.0, 0.0]
    res["obw_lo"], res["obw_hi"], res["xdb_lo"], res["xdb_hi"] = [10, -1, 0], [13, -1, 0], [11, -1, 0], [11, -1, 0]
    f = X.result_freqs(res, freqs)
    assert np.allclose(f["center_hz"][0], freqs[0] + 11.5 * step) and np.allclose(f["obw_hz"][0], 4 * step) and np.allclose(f["xdb_hz"][0], step)
    assert all(np.isnan(f[k][1:]).all() for k in f)
    main, adj = np.zeros(2, dtype=X.RESULT_DTYPE), np.zeros(2, dtype=X.RESULT_DTYPE)
    main["flags"], main["power"], adj["flags"], adj["power"] = [1, 1], [1.0, 1.0], [1, 0], [0.001, 0.001]
    got = X.acpr(main, adj)
    assert np.allclose(got[0], -30.0) and np.isnan(got[1])


# ------------------------------------------------------------------------------------------ command line
BASE = ["zeroSpan", "fftSize", "64", "xRes", "64"]
DET = ["detect", "8:2:6"]


def transcript(K, argv):
    d, out, exited = {}, io.StringIO(), False
    with contextlib.redirect_stdout(out):
        try:
            K.handle_args(d, BASE + argv)
        except SystemExit:
            exited = True
    return d, out.getvalue(), exited


def test_measure_key_parses_in_each_form(K):
    d, out, exited = transcript(K, DET + ["measure", "99"])
    assert not exited and out == "" and d["measure.plan"] == dict(percent=99.0, occupied=float(np.float32(0.99)), xdb=3.0, margin=0)
    d, out, exited = transcript(K, DET + ["measure", "99:xdb=6:margin=2", "measureSave", "x.npz"])
    assert not exited and out == "" and d["measure.plan"] == dict(percent=99.0, occupied=float(np.float32(0.99)), xdb=6.0, margin=2)
    d, out, exited = transcript(K, DET + ["MEASURE", "50:MARGIN=65536:XDB=0.5"])
    assert not exited and d["measure.plan"] == dict(percent=50.0, occupied=0.5, xdb=0.5, margin=65536) and d["measureSave"] == ""
    d, out, exited = transcript(K, DET + ["measure", "99.5:xdb=100", "track", "2:1"])
    assert not exited and d["measure.plan"]["xdb"] == 100.0 and d["track.spec"] is not None
    assert K._HANDLERS.index(K._handle_detect) < K._HANDLERS.index(K._handle_measure)
    assert "MEASURE" not in K._KEYS and sorted(K._KEYS_MEASURE) == ["MEASURE", "MEASURESAVE"]
    assert "`measure`" in K.__doc__ and "`measureSave`" in K.__doc__ and "power_net_db" in K.__doc__


@pytest.mark.parametrize("value", ["x", "49.9", "100", "101", "-1", "nan", "inf", "99.9999999999", "99:xdb", "99:xdb=x", "99:xdb=-1",
                                   "99:xdb=101", "99:xdb=nan", "99:margin=-1", "99:margin=65537", "99:margin=2.5", "99:margin=x",
                                   "99:xdb=3:xdb=4", "99:margin=1:margin=1", "99:bogus=1", "99:6", "99:"])
def test_measure_key_refuses_with_the_rule(K, value):
    d, out, exited = transcript(K, DET + ["measure", value])
    assert exited and d["cmd.stop"] is True and "measure.plan" not in d
    assert out == "ERROR:handle_args: measure [%s]: %s\n" % (value, K.MEASURE_RULE)


def test_measure_needs_detect_and_zero_span(K):
    d, out, exited = transcript(K, ["measure", "99"])
    assert exited and out == "ERROR:handle_args: measure [99] measures the emissions of detect: give [detect T:G:THR] as well\n"
    d, out, exited = transcript(K, ["measure", "x"])            # a bad text is told first, as track does
    assert exited and K.MEASURE_RULE in out
    for mode in (["scan", "startFreq", "100e6", "endFreq", "104.8e6"], ["fmScan"], ["quickFullScan"], ["zeroSpanSave"]):
        d, out, exited = transcript(K, mode + ["measure", "99"])
        assert exited and "measure [99] is zeroSpan only" in out and "measure.plan" not in d, mode
    d, out, exited = transcript(K, ["zeroSpanPlay"] + DET + ["measure", "99"])
    assert not exited and "measure.plan" not in d and "WARN:handle_args: measure [99] is ignored when playing saved spectra" in out
    d, out, exited = transcript(K, ["bUsePSD", "true", "measure", "99"])
    assert exited and out == "ERROR:handle_args: measure [99] needs bUsePSD false: it reads the engine's own dB rows\n"
    d, out, exited = transcript(K, ["bUsePSD", "true"] + DET + ["measure", "99"])
    assert exited and "detect [8:2:6] needs bUsePSD false" in out            # the detector's own refusal comes first


def test_an_absent_key_leaves_nothing_behind(K):
    d, out, exited = transcript(K, DET)
    plain, plain_out, _ = transcript(K, [])
    assert not exited and out == plain_out == ""
    assert sorted(k for k in d if k.lower().startswith("measure")) == ["measure", "measureSave"] and d["measure"] == d["measureSave"] == ""
    assert {k: K.defaults()[k] for k in ("measure", "measureSave")} == {"measure": "", "measureSave": ""}
    d, out, exited = transcript(K, DET + ["measureSave", "x.npz"])
    assert not exited and out == "WARN:handle_args: measureSave [x.npz] is ignored without measure\n" and "measure.plan" not in d
    stale = {"measure.plan": dict(percent=1.0)}                                # a dict that is used again does not keep an old plan
    K.handle_args(stale, BASE + DET)
    assert "measure.plan" not in stale
    d, out, exited = transcript(K, DET + ["measure"])
    assert exited and out == "ERROR:handle_args: Missing value for [MEASURE]\n"


# ------------------------------------------------------------------------------------------ the library's own kernel catalogue
def test_the_compiled_kernels_are_the_listed_ones_and_each_names_its_gpu_test(tmp_path):
    assert kernel_names(os.path.join(PKG_DIR, RECORD.so), tmp_path) == set(mm.KERNELS)
    for kernel, node in mm.KERNELS.items():
        path, func = node.split("::")
        text = open(os.path.join(ROOT, path)).read()
        assert re.search(r"^def %s\(" % re.escape(func), text, flags=re.M) and "pytest.mark.gpu" in text, node
