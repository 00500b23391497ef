"""Host side of the CFAR signal detector (no GPU needed): the companion header and library, the binding, the integer model every
GPU test compares against, the command line keys, and the kernels' resource report."""
import ctypes as C
import importlib
import json
import os
import re

import numpy as np
import pytest

import detect_model as dm
from companion_helper import BY_MODULE, check_header_exports_binding
from conftest import GOLDEN, ROOT, load_pkg
from test_isa_regression import _asm, _kernels, _resource

PKG_DIR = os.path.join(ROOT, "prgs-sdr-kspecanal_amd")
F = np.float32(-90.0)                      # the floor of the hand-written rows
STEP = np.float32(1.0 / 64.0)              # one quantisation step


@pytest.fixture(scope="module")
def X():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.detect")


@pytest.fixture(scope="module")
def K():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")


# ------------------------------------------------------------------------------------------ header, exports, binding
def test_header_is_c99_and_matches_the_exports_and_the_binding(X, tmp_path):
    extra = ('typedef kse_detector* handle;\ntypedef char size_is_32[sizeof(kse_emission) == 32 ? 1 : -1];\n'
             + "".join('typedef char off_%s[offsetof(kse_emission, %s) == %d ? 1 : -1];\n' % (f, f, o) for f, o in
                       (("row", 0), ("bin_lo", 8), ("bin_hi", 12), ("peak_bin", 16), ("ndet", 20), ("peak_db", 24),
                        ("floor_db", 28))))
    text, _ = check_header_exports_binding(BY_MODULE["detect"], X, tmp_path, extra,
                                           ["KSE_MAX_CAPACITY", "KSE_MODE_CA", "KSE_MODE_GO", "KSE_MODE_SO"])
    assert "KSE_ABI_VERSION 1" in text and X.ABI_VERSION == 1
    for name, value in (("KSE_MODE_CA", 0), ("KSE_MODE_GO", 1), ("KSE_MODE_SO", 2), ("KSE_MIN_NBINS", X.MIN_NBINS),
                        ("KSE_MAX_NBINS", X.MAX_NBINS), ("KSE_MAX_TRAIN", X.MAX_TRAIN), ("KSE_MAX_GUARD", X.MAX_GUARD),
                        ("KSE_MAX_GAP", X.MAX_GAP), ("KSE_MAX_CAPACITY", X.MAX_CAPACITY)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value, name
    assert X.MODES == dm.MODES == {"ca": 0, "go": 1, "so": 2}
    assert X.EMISSION_DTYPE == dm.EMISSION_DTYPE and X.EMISSION_DTYPE.itemsize == 32
    assert [X.EMISSION_DTYPE.fields[n][1] for n in X.EMISSION_DTYPE.names] == [0, 8, 12, 16, 20, 24, 28]


def test_the_frozen_boundaries_are_untouched(X):
    lib = importlib.import_module("prgs-sdr-kspecanal_amd._lib")
    others = [importlib.import_module("prgs-sdr-kspecanal_amd." + m) for m in ("density", "mask", "ddc")]
    assert len(lib.SIGNATURES) == 52 and lib.ABI_VERSION == 5
    assert [len(m.SIGNATURES) for m in others[:2]] == [14, 18] and all(m.ABI_VERSION == 1 for m in others[:2])
    assert not [n for m in [lib] + others for n in m.SIGNATURES if n.startswith("kse_")]
    assert all(n.startswith("kse_") for n in X.SIGNATURES)
    pkg = load_pkg()
    for name in ("SignalDetector", "EMISSION_DTYPE", "emission_freqs"):
        assert getattr(pkg, name) is getattr(X, name) and name in pkg.__all__, name


def test_library_loads_without_a_gpu_and_there_is_no_fallback(X):
    lib = X.load()
    assert lib.kse_abi_version() == X.ABI_VERSION
    try:
        import torch
        have_gpu = torch.cuda.is_available()
    except ImportError:
        have_gpu = False
    if not have_gpu:
        with pytest.raises(X.KsaError):
            X.SignalDetector(64, 8, 1, 10.0)
    with pytest.raises(X.KsaError, match="__graft_entry__"):
        X.load(os.path.join(PKG_DIR, "no_such_libksa_detect.so"))
    with pytest.raises(X.KsaError, match="mode"):
        X.SignalDetector(64, 8, 1, 10.0, mode="os")
    # create-time refusals need no device: each has its own text and leaves a null handle
    good = dict(device=0, nbins=64, train=8, guard=1, thr=10.0, mode=0, min_width=1, max_gap=0, capacity=16)
    texts = []
    for change, text in ((dict(nbins=15), "nbins 15"), (dict(nbins=16385), "nbins 16385"), (dict(train=0), "train 0"),
                         (dict(train=1025), "train 1025"), (dict(guard=-1), "guard -1"), (dict(guard=257), "guard 257"),
                         (dict(thr=-0.5), "threshold_db"), (dict(thr=100.5), "threshold_db"), (dict(thr=float("nan")), "threshold_db"),
                         (dict(thr=float("inf")), "threshold_db"), (dict(mode=3), "mode 3"), (dict(mode=-1), "mode -1"),
                         (dict(min_width=0), "min_width 0"), (dict(min_width=65), "min_width 65 exceeds"),
                         (dict(max_gap=-1), "max_gap -1"), (dict(max_gap=1025), "max_gap 1025"), (dict(capacity=0), "capacity 0"),
                         (dict(capacity=2 ** 20 + 1), "capacity"), (dict(device=-1), "device -1")):
        a = dict(good, **change)
        h = C.c_void_p(1)
        rc = lib.kse_create(a["device"], a["nbins"], a["train"], a["guard"], a["thr"], a["mode"], a["min_width"], a["max_gap"],
                            a["capacity"], C.byref(h))
        assert rc != 0 and h.value is None, text
        got = lib.kse_last_error().decode()
        assert text in got, (text, got)
        texts.append(re.sub(r"-?[0-9.]+|nan|inf", "#", got))
    # nbins / train / guard / threshold / mode / min_width < 1 / min_width > nbins / max_gap / capacity / device
    assert len(set(texts)) == 10, sorted(set(texts))
    assert lib.kse_create(0, 64, 8, 1, 10.0, 0, 1, 0, 16, None) != 0 and "null out" in lib.kse_last_error().decode()
    if not have_gpu:                            # every value at its limit is accepted; only a device is missing then
        for a in (dict(good, nbins=16, train=1024, guard=256, thr=0.0, min_width=16, max_gap=1024, capacity=2 ** 20),
                  dict(good, nbins=16384, thr=100.0, mode=2, min_width=16384)):
            h = C.c_void_p(1)
            assert lib.kse_create(a["device"], a["nbins"], a["train"], a["guard"], a["thr"], a["mode"], a["min_width"],
                                  a["max_gap"], a["capacity"], C.byref(h)) != 0 and h.value is None
            assert "hip" in lib.kse_last_error().decode()


def test_a_null_object_is_refused_by_every_entry_point(X):
    lib = X.load()
    n = C.c_int64()
    p = C.c_void_p()
    buf = (C.c_float * 16)()
    calls = {
        "kse_set_stream": lambda: lib.kse_set_stream(None, None),
        "kse_synchronize": lambda: lib.kse_synchronize(None),
        "kse_detect_rows_dev": lambda: lib.kse_detect_rows_dev(None, buf, 16, 1, None, None),
        "kse_detect_rows": lambda: lib.kse_detect_rows(None, buf, 1),
        "kse_set_params": lambda: lib.kse_set_params(None, 8, 1, 10.0, 0, 1, 0),
        "kse_set_row_base": lambda: lib.kse_set_row_base(None, 0),
        "kse_read_hits": lambda: lib.kse_read_hits(None, None, C.byref(n)),
        "kse_read_emissions": lambda: lib.kse_read_emissions(None, None, 0, C.byref(n), C.byref(n)),
        "kse_hits_dev": lambda: lib.kse_hits_dev(None, C.byref(p)),
        "kse_emissions_dev": lambda: lib.kse_emissions_dev(None, C.byref(p), C.byref(p)),
        "kse_merge_hits_dev": lambda: lib.kse_merge_hits_dev(None, buf, 0),
        "kse_clear_emissions": lambda: lib.kse_clear_emissions(None),
        "kse_reset": lambda: lib.kse_reset(None),
        "kse_kernel_info": lambda: lib.kse_kernel_info(None, None, None, None, None, None, None),
    }
    assert set(calls) == set(X.SIGNATURES) - {"kse_abi_version", "kse_last_error", "kse_create", "kse_destroy"}
    for name, call in calls.items():
        assert call() != 0 and "null detector" in lib.kse_last_error().decode(), name
    lib.kse_destroy(None)
    for name in ("detect_rows_dev", "detect_rows", "emissions", "hits", "occupancy", "hits_view", "set_params", "set_row_base",
                 "merge_hits_dev", "clear_emissions", "reset", "kernel_info", "close", "set_stream", "synchronize"):
        assert callable(getattr(X.SignalDetector, name)), name


# ------------------------------------------------------------------------------------------ the model checks itself
def flat(nbins, nrows=1):
    return np.full((nrows, nbins), F, dtype=np.float32)


def test_model_quantises_to_a_64th_of_a_db_to_nearest_even():
    x = np.array([[-90.0, -90.0 + 1 / 128, -90.0 + 3 / 128, 0.0078125, -0.0078125, 600.0, -600.0, np.inf, -np.inf, np.nan]], np.float32)
    q, valid = dm.quantise(x)
    assert q.tolist() == [[-5760, -5760, -5758, 0, 0, 32000, -32000, 32000, 0, 0]]       # halves go to the even neighbour
    assert valid.tolist() == [[True] * 8 + [False, False]]
    assert dm.threshold_q(10.0) == 640 and dm.threshold_q(0.0) == 0 and dm.threshold_q(0.0078125) == 0 and dm.threshold_q(100.0) == 6400


def test_model_equality_is_not_a_detection():
    rows = flat(32)
    assert dm.detect(rows, 4, 1, 0.0)["total"] == 0           # q*C == S everywhere
    rows[0, 10] = F + STEP
    r = dm.detect(rows, 4, 1, 0.0)
    assert np.flatnonzero(r["det0"][0]).tolist() == [10] and r["total"] == 1
    e = r["events"][0]
    assert (e["row"], e["bin_lo"], e["bin_hi"], e["peak_bin"], e["ndet"]) == (0, 10, 10, 10, 1)
    assert e["peak_db"] == F + STEP and e["floor_db"] == F
    for mode in ("go", "so"):
        assert np.flatnonzero(dm.detect(rows, 4, 1, 0.0, mode)["det0"][0]).tolist() == [10]


def test_model_threshold_is_exclusive():
    rows = flat(32)
    rows[0, 10] = F + np.float32(10.0)
    for mode in ("ca", "go", "so"):
        assert dm.detect(rows, 4, 1, 10.0, mode)["total"] == 0, mode
    rows[0, 10] += STEP
    for mode in ("ca", "go", "so"):
        r = dm.detect(rows, 4, 1, 10.0, mode)
        assert r["total"] == 1 and r["events"]["peak_bin"].tolist() == [10] and r["hits"][10] == 1 and r["hits"].sum() == 1, mode


def test_model_peak_tie_goes_to_the_lowest_bin():
    rows = flat(32)
    rows[0, 10:13] = -60.0
    r = dm.detect(rows, 4, 3, 10.0)
    e = r["events"]
    assert r["total"] == 1 and (e["bin_lo"][0], e["bin_hi"][0], e["peak_bin"][0], e["ndet"][0]) == (10, 12, 10, 3)
    rows[0, 12] = -59.0
    assert dm.detect(rows, 4, 3, 10.0)["events"]["peak_bin"].tolist() == [12]


def test_model_min_width_drops_narrow_runs_before_max_gap_bridges():
    rows = flat(64)
    rows[0, 5:8] = rows[0, 10] = rows[0, 13:16] = -60.0      # runs of 3, 1, 3 bins, two gaps of 2 bins
    args = (8, 12, 10.0, "ca")
    r = dm.detect(rows, *args, min_width=1, max_gap=0)
    assert np.flatnonzero(r["det0"][0]).tolist() == [5, 6, 7, 10, 13, 14, 15]
    assert [tuple(e) for e in r["events"][["bin_lo", "bin_hi"]].tolist()] == [(5, 7), (10, 10), (13, 15)]
    # opening first: bin 10 is gone, the gap between the two kept runs is 5 bins, too wide for max_gap 3
    r = dm.detect(rows, *args, min_width=2, max_gap=3)
    assert [tuple(e) for e in r["events"][["bin_lo", "bin_hi", "ndet"]].tolist()] == [(5, 7, 3), (13, 15, 3)]
    assert r["hits"].sum() == 6 and not r["keep"][0, 10]
    # max_gap 5 bridges it; bin 10 lies inside the emission but is no keep bin
    r = dm.detect(rows, *args, min_width=2, max_gap=5)
    assert [tuple(e) for e in r["events"][["bin_lo", "bin_hi", "ndet"]].tolist()] == [(5, 15, 6)]
    rows[0, 10] = -40.0                                       # the strongest bin of the row, but not a keep bin: never the peak
    r = dm.detect(rows, *args, min_width=2, max_gap=5)
    assert r["det0"][0, 10] and r["events"]["peak_bin"].tolist() == [5]


def test_model_a_bridged_gap_counts_in_hits_but_not_in_ndet():
    rows = flat(64, 2)
    rows[:, 5:8] = rows[:, 10] = rows[:, 13:16] = -60.0
    r = dm.detect(rows, 8, 12, 10.0, "ca", min_width=1, max_gap=2)
    assert [tuple(e) for e in r["events"][["row", "bin_lo", "bin_hi", "ndet"]].tolist()] == [(0, 5, 15, 7), (1, 5, 15, 7)]
    assert r["hits"][5:16].tolist() == [2] * 11 and r["hits"].sum() == 22 and r["count"].tolist() == [1, 1]
    assert r["final"][0, 8] and not r["keep"][0, 8]


def test_model_nan_and_minus_inf_are_excluded_and_plus_inf_detects():
    rows = flat(32)
    rows[0, 8], rows[0, 9], rows[0, 20] = np.nan, -np.inf, np.inf
    r = dm.detect(rows, 4, 0, 10.0)
    assert np.flatnonzero(r["det0"][0]).tolist() == [20] and r["total"] == 1
    e = r["events"][0]
    assert np.isposinf(e["peak_db"]) and e["floor_db"] == F and e["peak_bin"] == 20
    line = r["floor"][0]
    assert line[10] == F and line[7] == F and line[12] == F                       # bins 8 and 9 add nothing to any sum
    assert line[19] == np.float32((7 * -5760 + 32000) / 8) * dm.SCALE             # +inf counts as 500 dB
    all_bad = np.full((2, 32), np.nan, dtype=np.float32)
    all_bad[1] = -np.inf
    r = dm.detect(all_bad, 4, 0, 0.0)
    assert r["total"] == 0 and np.isnan(r["floor"]).all() and not r["hits"].any()
    lone = np.full((1, 32), np.nan, dtype=np.float32)
    lone[0, 5] = -20.0                                        # a valid bin without a valid training cell is never detected
    for mode in ("ca", "go", "so"):
        assert dm.detect(lone, 4, 0, 0.0, mode)["total"] == 0, mode


def test_model_go_and_so_next_to_a_strong_neighbour():
    rows = flat(64)
    rows[0, 20:40] = -50.0                                    # a strong block
    rows[0, 16] = -75.0                                       # a weak signal in front of it: lagging mean -90, leading mean -60
    rows[0, 45] = -40.0                                       # behind it: lagging mean -70, leading mean -90
    res = {m: dm.detect(rows, 8, 1, 10.0, m) for m in ("ca", "go", "so")}
    assert [bool(res[m]["det0"][0, 16]) for m in ("ca", "go", "so")] == [False, False, True]   # pooled mean -75: not 10 dB below
    assert [bool(res[m]["det0"][0, 20]) for m in ("ca", "go", "so")] == [True, False, True]    # the block's edge sees the block
    assert [bool(res[m]["det0"][0, 45]) for m in ("ca", "go", "so")] == [True, True, True]
    floor_at_45 = {m: float(res[m]["events"][res[m]["events"]["peak_bin"] == 45]["floor_db"][0]) for m in res}
    assert floor_at_45 == {"ca": -80.0, "go": -70.0, "so": -90.0}
    e = res["so"]["events"]
    assert float(e[e["peak_bin"] == 16]["floor_db"][0]) == -90.0
    tie = flat(64)
    tie[0, 30] = -40.0                                        # equal means: the lagging side, whose sum is the same number
    for m in ("go", "so"):
        assert dm.detect(tie, 8, 1, 10.0, m)["events"]["floor_db"].tolist() == [-90.0]
    edge = flat(64)
    edge[0, 0] = edge[0, 63] = -40.0                          # no lagging cell at bin 0, no leading cell at bin 63
    for m in ("ca", "go", "so"):
        r = dm.detect(edge, 8, 1, 10.0, m)
        assert r["events"]["peak_bin"].tolist() == [0, 63] and r["events"]["floor_db"].tolist() == [-90.0, -90.0], m


def test_model_a_window_wider_than_the_row():
    rows = flat(16)
    rows[0, 7] = -70.0
    r = dm.detect(rows, 1024, 0, 10.0)
    assert np.flatnonzero(r["det0"][0]).tolist() == [7] and r["events"]["floor_db"].tolist() == [-90.0]
    assert r["floor"][0, 0] == np.float32(14 * -5760 + -4480) / np.float32(15) * dm.SCALE
    r = dm.detect(rows, 1024, 256, 10.0)                      # the guard alone covers the row: no training cell anywhere
    assert r["total"] == 0 and np.isnan(r["floor"]).all()
    wide = flat(64)
    wide[0, 40] = -70.0
    r = dm.detect(wide, 1024, 256, 0.0)
    assert r["total"] == 0 and np.isnan(r["floor"]).all()


def test_model_capacity_keeps_the_first_records_in_order():
    rows = flat(64, 5)
    rows[:, 10] = rows[:, 40] = -60.0
    r = dm.detect(rows, 4, 1, 10.0, capacity=3, row_base=100)
    assert r["total"] == 10 and len(r["all"]) == 10 and r["count"].tolist() == [2] * 5
    assert [tuple(e) for e in r["events"][["row", "bin_lo"]].tolist()] == [(100, 10), (100, 40), (101, 10)]
    assert r["hits"][10] == r["hits"][40] == 5 and r["hits"].sum() == 10
    assert dm.emissions_equal(r["events"], r["all"][:3]) and not dm.emissions_equal(r["events"], r["all"][1:4])
    empty = dm.detect(rows[:0], 4, 1, 10.0)
    assert empty["total"] == 0 and empty["hits"].shape == (64,) and empty["events"].dtype == dm.EMISSION_DTYPE


def test_emission_freqs_gives_centre_and_width_in_hz(X):
    freqs = np.fft.fftshift(np.fft.fftfreq(64, 1 / 2.4e6) + 92e6)
    ev = np.zeros(2, dtype=dm.EMISSION_DTYPE)
    ev["bin_lo"], ev["bin_hi"] = [10, 32], [12, 32]
    for fn in (X.emission_freqs, dm.emission_freqs):
        center, width = fn(ev, freqs)
        assert np.allclose(center, [freqs[11], 92e6]) and np.allclose(width, [3 * 2.4e6 / 64, 2.4e6 / 64])


# ------------------------------------------------------------------------------------------ command line
def test_detect_key_parses_in_each_form(K):
    base = ["zeroSpan", "fftSize", "512", "detect"]
    s = K.handle_args({}, base + ["32:2:10"])["detect.spec"]
    assert s == dict(train=32, guard=2, threshold=10.0, mode="ca", min_width=1, max_gap=0, capacity=4096)
    s = K.handle_args({}, base + ["8:0:6.5:mode=GO:minWidth=3:maxGap=70:events=10", "detectSave", "/tmp/x.npz"])["detect.spec"]
    assert s == dict(train=8, guard=0, threshold=6.5, mode="go", min_width=3, max_gap=70, capacity=10)
    s = K.handle_args({}, base + ["1024:256:0:events=1048576:mode=so"])["detect.spec"]       # the suffixes in any order
    assert (s["train"], s["guard"], s["threshold"], s["mode"], s["capacity"]) == (1024, 256, 0.0, "so", 1 << 20)
    d = K.handle_args({}, ["zeroSpan", "fftSize", "512"])
    assert d["detect"] == "" and d["detectSave"] == "" and d["detect.spec"] is None


@pytest.mark.parametrize("value", ["x", "32", "32:2", "32:2:", "0:2:10", "1025:2:10", "32:-1:10", "32:257:10", "32:2:-1", "32:2:101",
                                   "32:2:nan", "32:2:inf", "2.5:2:10", "32:2:10:mode=xx", "32:2:10:mode", "32:2:10:minWidth=0",
                                   "32:2:10:minWidth=513", "32:2:10:maxGap=-1", "32:2:10:maxGap=1025", "32:2:10:events=0",
                                   "32:2:10:events=1048577", "32:2:10:events=3:events=4", "32:2:10:minWidth=x", "32:2:10:12",
                                   "32:2:10:gap=3"])
def test_detect_key_refuses_with_the_rule(K, value, capsys):
    d = {}
    with pytest.raises(SystemExit):
        K.handle_args(d, ["zeroSpan", "fftSize", "512", "detect", value])
    assert d["cmd.stop"] is True
    assert K.DETECT_RULE in capsys.readouterr().out


def test_detect_is_zerospan_only(K, capsys):
    for mode in (["scan", "startFreq", "100e6", "endFreq", "104.8e6"], ["fmScan"], ["quickFullScan"], ["zeroSpanSave"]):
        with pytest.raises(SystemExit):
            K.handle_args({}, mode + ["detect", "32:2:10"])
        assert "zeroSpan only" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        K.handle_args({}, ["zeroSpan", "bUsePSD", "true", "detect", "32:2:10"])
    assert "bUsePSD false" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        K.handle_args({}, ["zeroSpan", "fftSize", "32768", "detect", "32:2:10"])      # a row longer than one workgroup's LDS
    assert K.DETECT_RULE in capsys.readouterr().out
    d = K.handle_args({}, ["zeroSpanPlay", "fftSize", "512", "detect", "32:2:10"])
    assert d["detect.spec"] is None and "WARN" in capsys.readouterr().out
    d = K.handle_args({}, ["zeroSpan", "fftSize", "512", "detectSave", "/tmp/x.npz"])
    assert d["detect.spec"] is None and "detectSave" in capsys.readouterr().out
    d = K.handle_args({}, ["zeroSpan", "fftSize", "512", "detect", "32:2:10", "density", "64:-120:0", "mask", "flat:-50", "zoom", "4"])
    assert d["detect.spec"] is not None and d["density.spec"] == (64, -120.0, 0.0) and d["mask.spec"] is not None
    assert d["zoom.spec"] is not None                         # the four combine


def test_defaults_leave_the_reference_cases_alone(K):
    cli = json.load(open(os.path.join(GOLDEN, "cli_args.json")))
    for name, case in cli.items():
        d = K.handle_args({}, case["argv"] + ["prgLoopCnt", "0"])
        for k, want in case["d"].items():
            assert d[k] == want, (name, k)
        assert d["detect.spec"] is None and d["detect"] == "" and d["detectSave"] == ""


# ------------------------------------------------------------------------------------------ resources
def test_every_detect_kernel_runs_without_scratch(tmp_path):
    kernels = _kernels(_asm(os.path.join(PKG_DIR, "csrc_detect", "kse_api.hip"), str(tmp_path / "kse_api.s")))
    names = sorted(kernels)
    assert len([k for k in names if "row_kernel<" in k]) == 4, names
    for needle in ("row_kernel<true, true>", "row_kernel<true, false>", "row_kernel<false, true>", "row_kernel<false, false>",
                   "sum_kernel", "offset_kernel", "merge_kernel"):
        assert [k for k in names if needle in k], (needle, names)
    for k in names:
        assert _resource(kernels[k][1], "ScratchSize") == 0, k
