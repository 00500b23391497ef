"""Host side of the frequency-mask trigger (no GPU needed): the companion header and library, the binding, the float32 model
every GPU test compares against, the command line keys, and the kernels' resource report."""
import ctypes as C
import importlib
import json
import os
import re

import numpy as np
import pytest

import mask_model as mm
from companion_helper import BY_MODULE, check_header_exports_binding
from conftest import GOLDEN, ROOT, load_pkg
from test_isa_regression import _asm, _kernels, _resource

PKG_DIR = os.path.join(ROOT, "prgs-sdr-kspecanal_amd")


@pytest.fixture(scope="module")
def M():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.mask")


@pytest.fixture(scope="module")
def K():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")


# ------------------------------------------------------------------------------------------ header, exports, binding
def test_header_is_c99_and_matches_the_exports_and_the_binding(M, tmp_path):
    extra = ('typedef ksm_mask* handle;\ntypedef char size_is_32[sizeof(ksm_event) == 32 ? 1 : -1];\n'
             + "".join('typedef char off_%s[offsetof(ksm_event, %s) == %d ? 1 : -1];\n' % (f, f, o) for f, o in
                       (("row", 0), ("nover", 8), ("nunder", 12), ("nnan", 16), ("peak_bin", 20), ("peak_excess", 24),
                        ("peak_kind", 28))))
    check_header_exports_binding(BY_MODULE["mask"], M, tmp_path, extra, ["KSM_MAX_CAPACITY"])
    assert M.EVENT_DTYPE == mm.EVENT_DTYPE and M.EVENT_DTYPE.itemsize == 32
    assert [M.EVENT_DTYPE.fields[n][1] for n in M.EVENT_DTYPE.names] == [0, 8, 12, 16, 20, 24, 28]


def test_the_frozen_boundaries_are_untouched(M):
    lib = importlib.import_module("prgs-sdr-kspecanal_amd._lib")
    dens = importlib.import_module("prgs-sdr-kspecanal_amd.density")
    assert len(lib.SIGNATURES) == 52 and lib.ABI_VERSION == 5
    assert len(dens.SIGNATURES) == 14 and dens.ABI_VERSION == 1
    assert not [n for n in list(lib.SIGNATURES) + list(dens.SIGNATURES) if n.startswith("ksm_")]
    pkg = load_pkg()
    assert pkg.SpectrumMask is M.SpectrumMask and pkg.learn_mask is M.learn_mask
    assert "SpectrumMask" in pkg.__all__ and "learn_mask" in pkg.__all__


def test_library_loads_without_a_gpu_and_there_is_no_fallback(M):
    lib = M.load()
    assert lib.ksm_abi_version() == M.ABI_VERSION
    try:
        import torch
        have_gpu = torch.cuda.is_available()
    except ImportError:
        have_gpu = False
    if not have_gpu:
        with pytest.raises(M.KsaError):
            M.SpectrumMask(64, np.zeros(64, dtype=np.float32))
    with pytest.raises(M.KsaError, match="__graft_entry__"):
        M.load(os.path.join(PKG_DIR, "no_such_libksa_mask.so"))
    # create-time refusals need no device: each has its own text and leaves a null handle
    up = np.zeros(64, dtype=np.float32)
    nan_up, nan_lo, above = up.copy(), up.copy(), up.copy()
    nan_up[5] = nan_lo[6] = np.nan
    above[7] = 1.0
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    texts = []
    for args, text in (((0, 8, p(up), None, 1, 16), "nbins"), ((0, 2 ** 20 + 16, p(up), None, 1, 16), "nbins"),
                       ((0, 64, p(up), None, 0, 16), "min_bins 0"), ((0, 64, p(up), None, 65, 16), "min_bins 65 exceeds"),
                       ((0, 64, p(up), None, 1, 0), "capacity"), ((0, 64, p(up), None, 1, 2 ** 20 + 1), "capacity"),
                       ((0, 64, None, None, 1, 16), "null upper"), ((0, 64, p(nan_up), None, 1, 16), "upper[5] is NaN"),
                       ((0, 64, p(up), p(nan_lo), 1, 16), "lower[6] is NaN"), ((0, 64, p(up), p(above), 1, 16), "lower[7]")):
        h = C.c_void_p(1)
        assert lib.ksm_create(*args, C.byref(h)) != 0 and h.value is None, text
        got = lib.ksm_last_error().decode()
        assert text in got, (text, got)
        texts.append(re.sub(r"-?[0-9.e+]+", "#", got))
    assert len(set(texts)) == 8, texts              # nbins / min_bins < 1 / min_bins > nbins / capacity / null / 2 NaNs / lower > upper
    # infinities are allowed in either line; only a device is missing then
    if not have_gpu:
        inf = np.full(64, np.inf, dtype=np.float32)
        h = C.c_void_p(1)
        assert lib.ksm_create(0, 64, p(inf), p(-inf), 1, 16, C.byref(h)) != 0 and h.value is None
        assert "hip" in lib.ksm_last_error().decode()


# ------------------------------------------------------------------------------------------ the model checks itself
def test_model_tie_goes_to_the_lowest_bin():
    rows = np.full((2, 16), -100.0, dtype=np.float32)
    rows[0, [9, 3, 12]] = -40.0                               # the same excess three times
    rows[1, 4], rows[1, 11] = -130.0, -40.0                   # under by 10, over by 10: the lower bin wins, whatever its kind
    r = mm.check(rows, -50.0, -120.0)
    assert r["peak_bin"].tolist() == [3, 4] and r["peak_kind"].tolist() == [0, 1]
    assert r["peak_excess"].tolist() == [10.0, 10.0]
    assert r["nover"].tolist() == [3, 1] and r["nunder"].tolist() == [0, 1]
    assert r["hits"][0].sum() == 4 and r["hits"][1, 4] == 1 and r["total"] == 2


def test_model_infinite_lines_and_values():
    up = np.full(16, -50.0, dtype=np.float32)
    lo = np.full(16, -120.0, dtype=np.float32)
    up[0], lo[0] = np.inf, -np.inf                            # bin 0 disabled both ways
    up[1] = -np.inf                                           # anything finite is over by +inf
    lo[1] = -np.inf
    lo[2] = up[2] = -80.0                                     # a line of zero width
    rows = np.full((4, 16), -100.0, dtype=np.float32)
    rows[0, 0] = np.inf                                       # +inf under a +inf line: not over
    rows[0, 1] = -np.inf                                      # -inf at a -inf line: not over (equal), not under
    rows[0, 2] = -80.0                                        # exactly on both lines: neither
    rows[1, 0] = -np.inf                                      # -inf above a -inf lower line: not under
    rows[1, 2] = -100.0
    rows[2, 5], rows[2, 9] = np.inf, np.inf                   # two +inf excesses: bin 5
    rows[3, 7] = -np.inf                                      # under by +inf
    r = mm.check(rows, up, lo)
    assert r["nover"].tolist() == [0, 1, 3, 1] and r["nunder"].tolist() == [0, 1, 1, 2]
    assert r["peak_bin"].tolist() == [-1, 1, 1, 1] and np.isposinf(r["peak_excess"][1:]).all()
    assert r["peak_excess"][0] == 0 and r["peak_kind"].tolist() == [-1, 0, 0, 0]
    assert r["event"].tolist() == [False, True, True, True]
    q = mm.check(rows[2:3, :], np.full(16, -50.0, np.float32))
    assert q["peak_bin"].tolist() == [5] and np.isposinf(q["peak_excess"][0])


def test_model_nan_only_rows_are_events_without_a_peak():
    rows = np.full((3, 16), -100.0, dtype=np.float32)
    rows[1, [2, 8]] = np.nan
    r = mm.check(rows, -50.0, -120.0, min_bins=5)
    assert r["event"].tolist() == [False, True, False] and r["total"] == 1
    e = r["events"][0]
    assert (e["row"], e["nover"], e["nunder"], e["nnan"], e["peak_bin"], e["peak_excess"], e["peak_kind"]) == (1, 0, 0, 2, -1, 0.0, -1)
    assert r["hits"][2].tolist() == [0, 0, 1, 0, 0, 0, 0, 0, 1] + [0] * 7 and not r["hits"][:2].any()


def test_model_min_bins_and_capacity_keep_the_first_events_in_order():
    rows = np.full((12, 16), -100.0, dtype=np.float32)
    for i in range(12):
        rows[i, :i % 4] = -40.0                               # 0, 1, 2, 3 bins over, repeating
    r1 = mm.check(rows, -50.0, min_bins=1, row_base=100)
    r3 = mm.check(rows, -50.0, min_bins=3, capacity=2, row_base=100)
    assert r1["events"]["row"].tolist() == [101, 102, 103, 105, 106, 107, 109, 110, 111] and r1["total"] == 9
    assert r3["events"]["row"].tolist() == [103, 107] and r3["total"] == 3
    assert np.array_equal(r1["hits"], r3["hits"])             # hits do not depend on min_bins or on the capacity
    assert r1["hits"][0].sum() == r1["events"]["nover"].sum()
    assert mm.check(rows[:0], -50.0)["total"] == 0 and mm.check(rows[:0], -50.0)["hits"].shape == (3, 16)


def test_learn_mask_skips_nans_and_disables_all_nan_columns(M):
    rows = np.array([[-90.0, np.nan, -70.0, np.nan], [-95.0, -60.0, np.nan, np.nan]], dtype=np.float32)
    for fn in (M.learn_mask, mm.learn_mask):
        up = fn(rows, 6.0)
        assert up.dtype == np.float32 and up.tolist() == [-84.0, -54.0, -64.0, np.inf]
    big = (np.random.default_rng(1).standard_normal((50, 64)) * 7 - 90).astype(np.float32)
    assert np.array_equal(M.learn_mask(big, 3.3), big.max(axis=0) + np.float32(3.3))
    assert mm.check(big, M.learn_mask(big, 0.0))["total"] == 0       # a row never exceeds the line it taught


def test_occupancy_and_events_need_the_library_only_for_the_gpu(M):
    assert set(M.EVENT_DTYPE.names) == {"row", "nover", "nunder", "nnan", "peak_bin", "peak_excess", "peak_kind"}
    for name in ("check_rows_dev", "check_rows", "hits", "occupancy", "events", "hits_view", "set_mask", "set_row_base",
                 "merge_hits_dev", "clear_events", "reset", "kernel_info", "close"):
        assert callable(getattr(M.SpectrumMask, name)), name


# ------------------------------------------------------------------------------------------ command line
def test_mask_key_parses_in_each_form(K, tmp_path):
    base = ["zeroSpan", "fftSize", "512", "mask"]
    s = K.handle_args({}, base + ["flat:-50"])["mask.spec"]
    assert s["kind"] == "flat" and np.array_equal(s["upper"], np.full(512, -50, np.float32)) and s["lower"] is None
    assert (s["min_bins"], s["capacity"]) == (1, 4096)
    s = K.handle_args({}, base + ["flat:-50:-120:minBins=3:events=10", "maskSave", "/tmp/x.npz"])["mask.spec"]
    assert np.array_equal(s["lower"], np.full(512, -120, np.float32)) and (s["min_bins"], s["capacity"]) == (3, 10)
    s = K.handle_args({}, base + ["learn:5:6.5:events=7"])["mask.spec"]
    assert (s["kind"], s["frames"], s["margin"], s["min_bins"], s["capacity"]) == ("learn", 5, 6.5, 1, 7)
    one, two = tmp_path / "one.npy", tmp_path / "a:b.npy"
    np.save(one, np.linspace(-60, -40, 512).astype(np.float32))
    np.save(two, np.stack([np.full(512, -40.0), np.full(512, -130.0)]))
    s = K.handle_args({}, base + ["file:%s" % one])["mask.spec"]
    assert s["upper"].dtype == np.float32 and s["upper"][0] == -60 and s["lower"] is None
    s = K.handle_args({}, base + ["file:%s:minBins=2" % two])["mask.spec"]
    assert s["upper"][3] == -40 and s["lower"][3] == -130 and s["min_bins"] == 2
    d = K.handle_args({}, ["zeroSpan", "fftSize", "512"])
    assert d["mask"] == "" and d["maskSave"] == "" and d["mask.spec"] is None


@pytest.mark.parametrize("value", ["x", "flat", "flat:", "flat:nan", "flat:-50:-40", "flat:-50:-60:-70", "learn:0:6", "learn:5", "learn:5:inf",
                                   "learn:2.5:6", "file:", "file:/no/such/file.npy", "flat:-50:minBins=0", "flat:-50:minBins=513",
                                   "flat:-50:events=0", "flat:-50:events=1048577", "flat:-50:events=3:events=4", "flat:-50:minBins=x",
                                   "BADSHAPE", "HASNAN", "CROSSED"])
def test_mask_key_refuses_with_the_rule(K, value, capsys, tmp_path):
    if value == "BADSHAPE":
        np.save(tmp_path / "m.npy", np.zeros(511, dtype=np.float32))
    elif value == "HASNAN":
        np.save(tmp_path / "m.npy", np.full(512, np.nan, dtype=np.float32))
    elif value == "CROSSED":
        np.save(tmp_path / "m.npy", np.stack([np.full(512, -90.0), np.full(512, -80.0)]).astype(np.float32))
    if value.isupper():
        value = "file:%s" % (tmp_path / "m.npy")
    d = {}
    with pytest.raises(SystemExit):
        K.handle_args(d, ["zeroSpan", "fftSize", "512", "mask", value])
    assert d["cmd.stop"] is True
    assert K.MASK_RULE in capsys.readouterr().out


def test_mask_is_zerospan_only(K, capsys):
    for mode in (["scan", "startFreq", "100e6", "endFreq", "104.8e6"], ["fmScan"], ["quickFullScan"], ["zeroSpanSave"]):
        with pytest.raises(SystemExit):
            K.handle_args({}, mode + ["mask", "flat:-50"])
        assert "zeroSpan only" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        K.handle_args({}, ["zeroSpan", "bUsePSD", "true", "mask", "flat:-50"])
    assert "bUsePSD false" in capsys.readouterr().out
    d = K.handle_args({}, ["zeroSpanPlay", "fftSize", "512", "mask", "flat:-50"])
    assert d["mask.spec"] is None and "WARN" in capsys.readouterr().out
    d = K.handle_args({}, ["zeroSpan", "fftSize", "512", "mask", "flat:-50", "density", "64:-120:0"])      # the two combine
    assert d["mask.spec"] is not None and d["density.spec"] == (64, -120.0, 0.0)


def test_defaults_leave_the_reference_cases_alone(K):
    cli = json.load(open(os.path.join(GOLDEN, "cli_args.json")))
    for name, case in cli.items():
        d = K.handle_args({}, case["argv"] + ["prgLoopCnt", "0"])
        for k, want in case["d"].items():
            assert d[k] == want, (name, k)
        assert d["mask.spec"] is None and d["mask"] == "" and d["maskSave"] == ""


# ------------------------------------------------------------------------------------------ resources
def test_every_mask_kernel_runs_without_scratch(tmp_path):
    kernels = _kernels(_asm(os.path.join(PKG_DIR, "csrc_mask", "ksm_api.hip"), str(tmp_path / "ksm_api.s")))
    names = sorted(kernels)
    assert len([k for k in names if "check_kernel<" in k]) == 2, names
    for needle in ("check_kernel<true>", "check_kernel<false>", "count_kernel", "scatter_kernel", "merge_kernel"):
        assert [k for k in names if needle in k], (needle, names)
    for k in names:
        assert _resource(kernels[k][1], "ScratchSize") == 0, k
