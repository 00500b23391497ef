"""Host side of the emission tracker (no GPU needed): the companion header and library, the binding, the
model every GPU test compares against on hand-worked cases, and the `track` / `trackSave` keys of the command line."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import track_model as tm
from companion_helper import BY_MODULE, check_header_exports_binding
from conftest import ROOT, load_pkg

PKG_DIR = os.path.join(ROOT, "prgs-sdr-kspecanal_amd")
LIB = os.path.join(PKG_DIR, "libksa_track.so")
OFFSETS = {"row_first": 0, "row_last": 8, "peak_row": 16, "cells": 24, "sum_mid2": 32, "bin_lo": 40, "bin_hi": 44, "nspans": 48,
           "peak_bin": 52, "mid2_first": 56, "mid2_last": 60, "first_span": 64, "flags": 68, "peak_db": 72, "floor_db": 76}
SPAN_OFFSETS = {"row": 0, "bin_lo": 8, "bin_hi": 12, "peak_bin": 16, "ndet": 20, "peak_db": 24, "floor_db": 28}


@pytest.fixture(scope="module")
def X():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.track")


@pytest.fixture(scope="module")
def K():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")


# ------------------------------------------------------------------------------------------ header, exports, binding
def test_header_is_c99_and_matches_the_exports_and_the_binding(X, tmp_path):
    extra = ('typedef ktr_tracker* handle;\ntypedef char track_is_80_bytes[sizeof(ktr_track) == 80 ? 1 : -1];\n'
             'typedef char span_is_32_bytes[sizeof(ktr_span) == 32 ? 1 : -1];\n'
             + "".join('typedef char t_%s_at_%d[offsetof(ktr_track, %s) == %d ? 1 : -1];\n' % (f, o, f, o) for f, o in OFFSETS.items())
             + "".join('typedef char s_%s_at_%d[offsetof(ktr_span, %s) == %d ? 1 : -1];\n' % (f, o, f, o) for f, o in SPAN_OFFSETS.items()))
    text, _ = check_header_exports_binding(BY_MODULE["track"], X, tmp_path, extra,
                                           ["KTR_MAX_ROW_GAP", "KTR_MAX_NBINS", "KTR_MAX_SPANS", "KTR_MAX_CAPACITY", "KTR_FLAG_OPEN_END"])
    assert X.ABI_VERSION == 1
    for name, value in (("KTR_MAX_NBINS", X.MAX_NBINS), ("KTR_MAX_SPANS", X.MAX_SPANS), ("KTR_MAX_ROW_GAP", X.MAX_ROW_GAP),
                        ("KTR_MAX_CAPACITY", X.MAX_CAPACITY), ("KTR_FLAG_OPEN_END", X.FLAG_OPEN_END)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value, name
    assert (X.MAX_NBINS, X.MAX_SPANS, X.MAX_ROW_GAP, X.MAX_CAPACITY) == (2 ** 24, 2 ** 22, 1024, 2 ** 20)
    assert X.FLAG_OPEN_END == tm.FLAG_OPEN_END == 1
    # the records: the binding's dtypes, the model's and the header's structs are one layout
    assert X.TRACK_DTYPE == tm.TRACK_DTYPE and X.TRACK_DTYPE.itemsize == 80
    assert {n: X.TRACK_DTYPE.fields[n][1] for n in X.TRACK_DTYPE.names} == OFFSETS == X.TRACK_OFFSETS
    fields = re.search(r"typedef struct ktr_track \{(.*?)\} ktr_track;", text, re.S).group(1)
    assert re.findall(r"(?:int64_t|int32_t|float)\s+(\w+);", fields) == list(X.TRACK_DTYPE.names)
    detect = importlib.import_module("prgs-sdr-kspecanal_amd.detect")
    assert X.SPAN_DTYPE == detect.EMISSION_DTYPE == tm.SPAN_DTYPE and X.SPAN_DTYPE.itemsize == 32
    assert {n: X.SPAN_DTYPE.fields[n][1] for n in X.SPAN_DTYPE.names} == SPAN_OFFSETS
    fields = re.search(r"typedef struct ktr_span \{(.*?)\} ktr_span;", text, re.S).group(1)
    assert re.findall(r"(?:int64_t|int32_t|float)\s+(\w+);", fields) == list(X.SPAN_DTYPE.names)
    # the span is the detector's record, field for field, although no header includes the other
    theirs = re.search(r"typedef struct kse_emission \{(.*?)\} kse_emission;", open(os.path.join(ROOT, "include", "ksa_detect.h")).read(), re.S)
    assert re.findall(r"(int64_t|int32_t|float)\s+(\w+);", theirs.group(1)) == re.findall(r"(int64_t|int32_t|float)\s+(\w+);", fields)
    assert "ksa_detect.h" not in re.sub(r"/\*.*?\*/", "", text, flags=re.S) and "#include <stdint.h>" in text
    assert "Out of scope" in text and "incremental" in text and "several GPUs" in text


def test_the_other_bindings_hold_no_ktr_name_and_the_package_exports_the_class(X):
    others = [importlib.import_module("prgs-sdr-kspecanal_amd." + m)
              for m in ("_lib", "density", "mask", "ddc", "detect", "demod", "chan", "resamp", "corr", "pulse")]
    assert not [n for m in others for n in m.SIGNATURES if n.startswith("ktr_")]
    assert all(n.startswith("ktr_") for n in X.SIGNATURES)
    pkg = load_pkg()
    assert pkg.EmissionTracker is X.EmissionTracker and pkg.TRACK_DTYPE is X.TRACK_DTYPE and pkg.SPAN_DTYPE is X.SPAN_DTYPE
    assert pkg.track_times_freqs is X.track_times_freqs and pkg.FLAG_OPEN_END == X.FLAG_OPEN_END == 1
    assert {"EmissionTracker", "TRACK_DTYPE", "SPAN_DTYPE", "FLAG_OPEN_END", "track_times_freqs"} <= set(pkg.__all__)
    for name in ("link", "link_dev", "link_detector", "tracks", "labels", "counts", "clear", "set_params", "tracks_view",
                 "counters_view", "kernel_info", "set_stream", "synchronize", "close"):
        assert callable(getattr(X.EmissionTracker, name)), name
    companion = importlib.import_module("prgs-sdr-kspecanal_amd._companion")
    engine = importlib.import_module("prgs-sdr-kspecanal_amd.engine")
    assert issubclass(X.EmissionTracker, companion.Companion) and isinstance(X._bind, companion.Binding) and X.DevArray is engine.DevArray
    assert X.KsaError is importlib.import_module("prgs-sdr-kspecanal_amd._lib").KsaError
    assert X.LIB_PATH == LIB and callable(X.load) and callable(X.lib) and callable(X.check)
    assert X.EmissionTracker._info_fields == ("threads", "lds_bytes", "vgprs", "grid", "launches")


def test_library_loads_without_a_gpu_and_every_refusal_has_its_own_text(X):
    lib = X.load()
    assert lib.ktr_abi_version() == X.ABI_VERSION
    try:
        import torch
        have_gpu = torch.cuda.is_available()
    except ImportError:
        have_gpu = False
    if not have_gpu:
        with pytest.raises(X.KsaError):
            X.EmissionTracker(1024)
    missing = os.path.join(PKG_DIR, "no_such_libksa_track.so")
    with pytest.raises(X.KsaError) as e:
        X.load(missing)
    assert str(e.value) == ("libksa_track.so is missing at %s -- build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950); "
                            "there is no CPU fallback" % missing)
    texts = []
    # (device, nbins, max_spans, row_gap, bin_slop, min_rows, min_spans, capacity)
    ok = (0, 1024, 4096, 1, 2, 1, 1, 16)

    def with_(**kw):
        names = ("device", "nbins", "max_spans", "row_gap", "bin_slop", "min_rows", "min_spans", "capacity")
        return tuple(kw.get(n, v) for n, v in zip(names, ok))

    for args, text in ((with_(nbins=0), "nbins 0 outside 1..16777216"), (with_(nbins=2 ** 24 + 1), "nbins 16777217 outside"),
                       (with_(max_spans=0), "max_spans 0 outside 1..4194304"), (with_(max_spans=2 ** 22 + 1), "max_spans 4194305 outside"),
                       (with_(row_gap=-1), "row_gap -1 outside 0..1024"), (with_(row_gap=1025), "row_gap 1025 outside"),
                       (with_(bin_slop=-1), "bin_slop -1 outside"), (with_(bin_slop=1025), "bin_slop 1025 outside 0..nbins = 1024"),
                       (with_(min_rows=0), "min_rows 0 must be >= 1"), (with_(min_rows=-5), "min_rows -5 must be >= 1"),
                       (with_(min_spans=0), "min_spans 0 must be >= 1"),
                       (with_(capacity=0), "track capacity 0 outside 1..1048576"), (with_(capacity=2 ** 20 + 1), "track capacity 1048577 outside"),
                       (with_(device=-1), "device -1 must be >= 0")):
        h = C.c_void_p(1)
        assert lib.ktr_create(*args, C.byref(h)) != 0 and h.value is None, text
        got = lib.ktr_last_error().decode()
        assert text in got, (text, got)
        texts.append(re.sub(r"-?[0-9]+", "#", got))
    # nbins / max_spans / row_gap / bin_slop / min_rows / min_spans / capacity / device
    assert len(set(texts)) == 8, sorted(set(texts))
    assert lib.ktr_create(*ok, None) != 0 and "null out pointer" in lib.ktr_last_error().decode()
    if not have_gpu:                                    # every parameter in range (bin_slop = nbins included): only a device is missing
        h = C.c_void_p(1)
        assert lib.ktr_create(*with_(bin_slop=1024, row_gap=1024, nbins=2 ** 24, capacity=2 ** 20), C.byref(h)) != 0 and h.value is None
        assert "hip" in lib.ktr_last_error().decode()
    # a null object is refused by every entry point that takes one, before anything else is looked at
    calls = (lambda: lib.ktr_set_stream(None, None), lambda: lib.ktr_synchronize(None),
             lambda: lib.ktr_set_params(None, 0, 0, 1, 1), lambda: lib.ktr_link_dev(None, None, -1, None, -1, None),
             lambda: lib.ktr_link(None, None, -1, -1, None), lambda: lib.ktr_read_tracks(None, None, -1, None, None, None, None),
             lambda: lib.ktr_read_labels(None, None, -1, None), lambda: lib.ktr_tracks_dev(None, None, None),
             lambda: lib.ktr_clear(None), lambda: lib.ktr_kernel_info(None, None, None, None, None, None))
    for call in calls:
        assert call() != 0 and lib.ktr_last_error().decode() == "null tracker object"
    lib.ktr_destroy(None)
    assert len(X.SIGNATURES) == len(calls) + 4          # those, abi_version, last_error, create, destroy
    # the per-call refusals come before any HIP call in the source: each text stands in front of the first HIP_OK of its function
    src = open(os.path.join(PKG_DIR, "csrc_track", "ktr_api.hip")).read()
    for fn, wants in (("ktr_link_dev", ("n_max %lld must be >= 0", "exceeds max_spans", "row_end %lld must be >= 0", "null spans pointer")),
                      ("ktr_link", ("n %lld must be >= 0", "exceeds max_spans", "row_end %lld must be >= 0", "null spans pointer", "is not valid")),
                      ("ktr_read_tracks", ("max_records %lld must be >= 0", "null records and count pointers")),
                      ("ktr_read_labels", ("max_labels %lld must be >= 0",)), ("ktr_tracks_dev", ("null records and counters out pointers",))):
        body = src[src.index("\nint %s(" % fn):]
        body = body[:body.index("\n}\n")]
        first_hip = body.find("DeviceGuard") if "DeviceGuard" in body else len(body)
        for w in wants:
            assert 0 <= body.find(w) < first_hip, (fn, w)


def test_the_track_sources_name_no_other_library_and_hold_no_float_atomic():
    for f in ("ktr_api.hip", "ktr_kernels.hpp"):
        text = open(os.path.join(PKG_DIR, "csrc_track", f)).read()
        assert "kse_" not in text and "ksa_detect.h" not in text
        assert not re.search(r"atomic\w*\([^;]*float", text)


# ------------------------------------------------------------------------------------------ the model on hand-worked cases
def _link(rows, nbins=64, row_end=None, **kw):
    s = tm.spans_of(rows)
    end = (max(r[0] for r in rows) + 1 if rows else 0) if row_end is None else row_end
    return tm.link(s, nbins, end, **kw)


def test_a_gap_of_exactly_one_plus_row_gap_rows_links_and_one_more_does_not():
    assert _link([(0, 5, 6), (1, 5, 6)])[1:3] == (1, 1)
    assert _link([(0, 5, 6), (2, 5, 6)])[1:3] == (2, 2)                  # row_gap 0: the next row only
    assert _link([(0, 5, 6), (4, 5, 6)], row_gap=3)[1:3] == (1, 1)       # 4 = 1 + 3
    assert _link([(0, 5, 6), (5, 5, 6)], row_gap=3)[1:3] == (2, 2)
    rec = _link([(0, 5, 6), (4, 5, 8)], row_gap=3)[0]
    assert (rec["row_first"][0], rec["row_last"][0], rec["nspans"][0], rec["cells"][0], rec["sum_mid2"][0]) == (0, 4, 2, 6, 24)
    assert (rec["bin_lo"][0], rec["bin_hi"][0], rec["mid2_first"][0], rec["mid2_last"][0], rec["first_span"][0]) == (5, 8, 11, 13, 0)


def test_slop_at_the_exact_bin_links_and_one_bin_farther_does_not():
    assert _link([(0, 5, 6), (1, 7, 9)])[1] == 2                         # abutting bins do not overlap
    assert _link([(0, 5, 6), (1, 7, 9)], bin_slop=1)[1] == 1
    assert _link([(0, 5, 6), (1, 8, 9)], bin_slop=1)[1] == 2
    assert _link([(0, 5, 6), (1, 8, 9)], bin_slop=2)[1] == 1
    assert _link([(0, 8, 9), (1, 5, 6)], bin_slop=1)[1] == 2             # and the same to the left
    assert _link([(0, 8, 9), (1, 5, 6)], bin_slop=2)[1] == 1
    assert _link([(0, 5, 6), (1, 6, 6)])[1] == 1                         # one shared bin


def test_spans_of_one_row_join_only_through_a_later_row():
    rows = [(0, 2, 3), (0, 10, 11), (1, 3, 10)]
    rec, total, comps, labels, bad = _link(rows)
    assert (total, comps, bad) == (1, 1, 0) and list(labels) == [0, 0, 0]
    assert (rec["first_span"][0], rec["nspans"][0], rec["bin_lo"][0], rec["bin_hi"][0]) == (0, 3, 2, 11)
    assert _link(rows[:2])[1] == 2 and _link([(0, 2, 3), (0, 4, 5)], bin_slop=5)[1] == 2       # never within a row
    # a comb that joins in its last row: the lowest index is the id of all
    comb = [(r, 10 * t, 10 * t + 1) for r in range(3) for t in range(4)] + [(3, 0, 31)]
    rec, total, comps, labels, _ = _link(comb)
    assert (total, comps) == (1, 1) and set(labels) == {0} and rec["first_span"][0] == 0 and rec["nspans"][0] == 13
    assert _link(comb[:-1])[1] == 4


def test_the_peak_span_its_ties_and_the_order_of_bit_patterns():
    vals = [-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf]
    keys = [tm.key(np.float32(v)) for v in vals]
    assert keys == sorted(keys) and len(set(keys)) == 6
    assert tm.key(np.float32(np.nan)) > tm.key(np.float32(np.inf))       # the positive quiet NaN orders last: no special case
    assert tm.key(np.float32(0.0)) == 0x80000000 and tm.key(np.float32(-0.0)) == 0x7FFFFFFF
    rows = [(0, 5, 6, -50.0, -70.0, 5), (1, 5, 6, -40.0, -71.0, 6), (2, 5, 6, -40.0, -72.0, 5), (3, 5, 6, -45.0, -73.0, 6)]
    rec = _link(rows)[0]
    assert (rec["peak_row"][0], rec["peak_bin"][0], rec["peak_db"][0], rec["floor_db"][0]) == (1, 6, -40.0, -71.0)   # the tie: lower index
    rows[3] = (3, 5, 6, -0.0, -73.0, 6)
    rows[1] = (1, 5, 6, 0.0, -71.0, 6)
    rec = _link(rows)[0]
    assert rec["peak_row"][0] == 1 and not np.signbit(rec["peak_db"][0])  # +0 beats -0
    rows[2] = (2, 5, 6, np.nan, -72.0, 5)
    rec = _link(rows)[0]
    assert rec["peak_row"][0] == 2 and np.isnan(rec["peak_db"][0]) and rec["floor_db"][0] == -72.0


def test_open_end_at_the_exact_row_end():
    rows = [(0, 5, 6), (1, 5, 6)]
    assert _link(rows, row_end=2)[0]["flags"][0] == tm.FLAG_OPEN_END      # row 2 has not arrived: it could join
    assert _link(rows, row_end=3)[0]["flags"][0] == 0
    assert _link(rows, row_end=3, row_gap=1)[0]["flags"][0] == tm.FLAG_OPEN_END
    assert _link(rows, row_end=4, row_gap=1)[0]["flags"][0] == 0


def test_filters_labels_beyond_capacity_and_bad_input():
    rows = [(0, 1, 1), (0, 5, 6), (0, 20, 21), (1, 5, 6), (1, 20, 25), (2, 5, 5), (2, 30, 30)]
    rec, total, comps, labels, bad = _link(rows)
    assert (total, comps, bad) == (4, 4, 0) and list(labels) == [0, 1, 2, 1, 2, 1, 3]
    assert list(rec["first_span"]) == [0, 1, 2, 6] and list(rec["nspans"]) == [1, 3, 2, 1]
    rec, total, comps, labels, _ = _link(rows, min_rows=2)
    assert (total, comps) == (2, 4) and list(labels) == [-1, 0, 1, 0, 1, 0, -1] and list(rec["first_span"]) == [1, 2]
    rec, total, comps, labels, _ = _link(rows, min_spans=3)
    assert (total, comps) == (1, 4) and list(labels) == [-1, 0, -1, 0, -1, 0, -1]
    rec, total, comps, labels, _ = _link(rows, capacity=2)                # ranks go on beyond the buffer
    assert (len(rec), total) == (2, 4) and list(labels) == [0, 1, 2, 1, 2, 1, 3] and list(rec["first_span"]) == [0, 1]
    # bad input: nothing is linked
    for broken, count in (([(1, 5, 6), (0, 5, 6)], 1), ([(0, 5, 9), (0, 9, 12)], 1), ([(0, 5, 6), (0, 5, 6)], 1),
                          ([(0, 7, 6)], 1), ([(0, -1, 6)], 1), ([(0, 60, 64)], 1), ([(-1, 5, 6), (0, 5, 6)], 1),
                          ([(0, 5, 6), (1, 5, 6), (1, 2, 3), (0, 9, 9)], 2)):
        rec, total, comps, labels, bad = _link(broken, row_end=10)
        assert bad == count and (len(rec), total, comps) == (0, 0, 0) and set(labels) == {-1}, broken
    assert _link([(0, 5, 6), (3, 5, 6)], row_end=3)[4] == 1               # row >= row_end
    rec, total, comps, labels, bad = _link([], row_end=0)               # an empty list is a good list
    assert (len(rec), total, comps, len(labels), bad) == (0, 0, 0, 0, 0)


def test_the_random_mix_holds_singletons_and_components_of_dozens_of_spans():
    s = tm.random_occupancy(1200, 64, 0.18, seed=5)
    assert 9000 < len(s) < 13000 and not len(tm.bad_indices(s, 64, 1200))
    rec, total, comps, labels, bad = tm.link(s, 64, 1200, row_gap=1, bin_slop=1, capacity=1 << 20)
    assert bad == 0 and total == comps == len(rec) and labels.min() == 0 and labels.max() == total - 1
    assert np.count_nonzero(rec["nspans"] == 1) > 50 and rec["nspans"].max() >= 24
    assert rec["nspans"].sum() == len(s) and np.all(np.diff(rec["first_span"]) > 0)
    assert np.array_equal(np.bincount(labels), rec["nspans"])


def test_track_times_freqs_matches_the_model(X):
    rows = [(10, 100, 104), (11, 101, 105), (12, 102, 106), (12, 300, 300), (20, 7, 7)]
    rec = _link(rows, nbins=1024)[0]
    freqs = np.fft.fftshift(np.fft.fftfreq(1024, 1 / 2.048e6)) + 100e6
    got, want = X.track_times_freqs(rec, freqs, 0.0005), tm.times_freqs(rec, freqs, 0.0005)
    assert sorted(got) == sorted(want) == ["center_hz", "drift_hz_per_s", "duration_s", "t_start_s", "width_hz"]
    for k in want:
        assert np.allclose(got[k], want[k], rtol=1e-12, atol=0), k
    assert np.allclose([got["t_start_s"][0], got["duration_s"][0], got["width_hz"][0]], [0.005, 0.0015, 7 * 2000.0], rtol=1e-12, atol=0)
    assert abs(got["drift_hz_per_s"][0] - 2 * 2000.0 / 0.001) < 1e-6     # two bins in two rows
    assert got["drift_hz_per_s"][1] == 0.0 and got["drift_hz_per_s"][2] == 0.0       # one-row tracks
    assert len(X.track_times_freqs(rec[:0], freqs, 0.0005)["center_hz"]) == 0


# ------------------------------------------------------------------------------------------ command line
BASE = ["zeroSpan", "fftSize", "1024", "samplingRate", "2048000"]
DET = ["detect", "16:2:10"]


def test_track_key_parses(K, capsys):
    d = K.handle_args({}, BASE + DET + ["track", "1:2"])
    assert d["track.spec"] == dict(row_gap=1, bin_slop=2, min_rows=1, min_spans=1, capacity=4096)
    assert "WARN" not in capsys.readouterr().out
    s = K.handle_args({}, BASE + DET + ["TRACK", "0:0:MINROWS=3:minSpans=4:events=9", "trackSave", "x.npz"])["track.spec"]
    assert s == dict(row_gap=0, bin_slop=0, min_rows=3, min_spans=4, capacity=9)
    s = K.handle_args({}, BASE + DET + ["track", "1024:1024:events=1048576:minRows=2"])["track.spec"]     # any order
    assert s == dict(row_gap=1024, bin_slop=1024, min_rows=2, min_spans=1, capacity=2 ** 20)
    d = K.handle_args({}, BASE)
    assert d["track"] == "" and d["trackSave"] == "" and d["track.spec"] is None
    capsys.readouterr()
    d = K.handle_args({}, BASE + DET + ["trackSave", "x.npz"])
    assert d["track.spec"] is None and "WARN:handle_args: trackSave [x.npz] is ignored without track" in capsys.readouterr().out


@pytest.mark.parametrize("text", ["1", "1:", ":2", "x:2", "1:y", "1.5:2", "-1:2", "1025:2", "1:-1", "1:1025", "1:2:minRows=0",
                                  "1:2:minSpans=0", "1:2:events=0", "1:2:events=1048577", "1:2:events", "1:2:minRows",
                                  "1:2:capacity=3", "1:2:3", "1:2:minRows=2:minRows=3", "1:2:events=3:events=3", "1:2:minRows=x",
                                  "1:2:minSpans=2:MINSPANS=2", "1:2:"])
def test_track_key_refuses_with_the_rule(K, text, capsys):
    d = {}
    with pytest.raises(SystemExit):
        K.handle_args(d, BASE + DET + ["track", text])
    assert d["cmd.stop"] is True
    assert K.TRACK_RULE in capsys.readouterr().out


def test_track_key_refuses_modes_and_a_missing_detector_each_with_its_own_text(K, capsys):
    with pytest.raises(SystemExit):
        K.handle_args({}, BASE + ["track", "1:2"])
    assert "ERROR:handle_args: track [1:2] links the emissions of detect: give [detect T:G:THR] as well" in capsys.readouterr().out
    for mode in (["scan", "startFreq", "100e6", "endFreq", "104.8e6"], ["fmScan"], ["quickFullScan"], ["zeroSpanSave"]):
        with pytest.raises(SystemExit):
            K.handle_args({}, mode + ["track", "1:2"])
        assert "track [1:2] is zeroSpan only" in capsys.readouterr().out
    d = K.handle_args({}, ["zeroSpanPlay", "fftSize", "512", "track", "1:2"])
    assert d["track.spec"] is None and "track [1:2] is ignored when playing saved spectra" in capsys.readouterr().out
    for front in (["zoom", "8"], ["channels", "8"]):                     # behind a front end the tracker is allowed
        assert K.handle_args({}, BASE + front + DET + ["track", "1:2"])["track.spec"] is not None
