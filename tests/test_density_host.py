"""Host side of the density (persistence) histogram (no GPU needed): the companion header and library, the binding, the
float32 model every GPU test compares against, the command line keys, and the add kernels' ISA."""
import importlib
import json
import os

import numpy as np
import pytest

import density_model as dm
from companion_helper import BY_MODULE, check_header_exports_binding
from conftest import GOLDEN, ROOT, load_pkg
from test_isa_regression import _asm, _find, _kernels, _mix, _resource

PKG_DIR = os.path.join(ROOT, "prgs-sdr-kspecanal_amd")


@pytest.fixture(scope="module")
def D():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.density")


@pytest.fixture(scope="module")
def K():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")


# ------------------------------------------------------------------------------------------ header, exports, binding
def test_header_is_c99_and_matches_the_exports_and_the_binding(D, tmp_path):
    check_header_exports_binding(BY_MODULE["density"], D, tmp_path, "typedef ksd_density* handle;\n", ["KSD_MAX_LEVELS"])


def test_the_frozen_boundary_is_untouched(D):
    lib = importlib.import_module("prgs-sdr-kspecanal_amd._lib")
    assert len(lib.SIGNATURES) == 52 and lib.ABI_VERSION == 5
    assert not [n for n in lib.SIGNATURES if n.startswith("ksd_")]
    pkg = load_pkg()
    assert pkg.SpectrumDensity is D.SpectrumDensity and "SpectrumDensity" in pkg.__all__


def test_library_loads_without_a_gpu_and_there_is_no_fallback(D):
    lib = D.load()
    assert lib.ksd_abi_version() == D.ABI_VERSION
    try:
        import torch
        have_gpu = torch.cuda.is_available()
    except ImportError:
        have_gpu = False
    if not have_gpu:
        with pytest.raises(D.KsaError):
            D.SpectrumDensity(64)
    with pytest.raises(D.KsaError, match="__graft_entry__"):
        D.load(os.path.join(PKG_DIR, "no_such_libksa_density.so"))
    # create-time refusals need no device: each has its own text and leaves a null handle
    import ctypes as C
    for args, text in (((0, 8, 8, 4, -1.0, 0.0), "nbins"), ((0, 64, 0, 4, -1.0, 0.0), "width"), ((0, 64, 48, 4, -1.0, 0.0), "divide"),
                       ((0, 64, 64, 0, -1.0, 0.0), "levels"), ((0, 64, 64, 4, 0.0, 0.0), "lo_db")):
        h = C.c_void_p(1)
        assert lib.ksd_create(*args, C.byref(h)) != 0 and h.value is None
        assert text in lib.ksd_last_error().decode()


# ------------------------------------------------------------------------------------------ the model checks itself
def test_model_column_sums(D):
    rng = np.random.default_rng(5)
    rows = (-90 + 6 * rng.standard_normal((37, 64))).astype(np.float32)
    rows[3, 5], rows[4, 6], rows[5, 7] = np.nan, np.inf, -np.inf
    for width in (64, 16, 1):
        c = dm.histogram(rows, width, 50, -120.0, -60.0)
        assert c.dtype == np.int64 and c.shape == (51, width)
        assert np.array_equal(c.sum(axis=0), np.full(width, 37 * (64 // width)))
    assert dm.histogram(rows, 64, 50, -120.0, -60.0)[50].sum() == 1


@pytest.mark.parametrize("levels,lo,hi", [(64, -120.0, 0.0), (256, -140.0, 0.0), (1000, -133.3, 7.1), (1, -1.0, 1.0), (7, 0.1, 0.7)])
def test_model_edges_land_where_the_formula_says(levels, lo, hi):
    """Values on lo, hi, every nominal edge and one float32 ulp either side: the model equals the header's formula evaluated
    value by value in Python with np.float32 scalars."""
    v = dm.edge_values(levels, lo, hi)
    got = dm.level_rows(v, levels, lo, hi)
    lo32, inv = np.float32(lo), np.float32(levels) / (np.float32(hi) - np.float32(lo))
    for x, row in zip(v, got):
        t = np.float32(np.float32(x - lo32) * inv)
        want = levels - 1 if t >= np.float32(levels) else 0 if t < 0 else int(t)
        assert row == want, (x, t, row, want)
    assert got[0] == 0                                    # exactly lo: t = 0
    assert got[levels] == levels - 1                      # exactly hi: t >= L (or rounds just below it) -- the last level either way
    below_lo = dm.level_rows(np.nextafter(np.float32(lo), np.float32(-np.inf)), levels, lo, hi)
    assert below_lo == 0
    assert np.all(np.diff(dm.level_rows(np.sort(v), levels, lo, hi)) >= 0)     # monotone in the value


def test_model_infinities_and_nan():
    v = np.array([-np.inf, np.inf, np.nan, -1e30, 1e30, -0.0, 0.0], dtype=np.float32)
    assert dm.level_rows(v, 10, -5.0, 5.0).tolist() == [0, 9, 10, 0, 9, 5, 5]


def test_model_decay_is_the_exact_floor():
    c = np.array([0, 1, 2, 3, 7, 2 ** 33 + 5, 2 ** 62 + 12345], dtype=np.int64)
    for num, den in ((3, 4), (0, 1), (1, 3), (2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 2, 2 ** 31 - 1)):
        want = [int(x) * num // den for x in c.tolist()]
        assert dm.decay(c, num, den).tolist() == want


def test_image_and_level_edges(D):
    e = D.level_edges(4, -100.0, -60.0)
    assert e.dtype == np.float64 and e.tolist() == [-100.0, -90.0, -80.0, -70.0, -60.0]
    counts = np.array([[0, 4], [2, 0], [8, 0], [99, 99]], dtype=np.int64)     # last row: NaNs
    img = D.image(counts)
    assert img.dtype == np.float32 and img.shape == (3, 2)
    assert img.tolist() == [[0.0, 1.0], [0.25, 0.0], [1.0, 0.0]]
    assert D.image(counts, normalize="max").tolist() == [[0.0, 0.5], [0.25, 0.0], [1.0, 0.0]]
    assert D.image(counts, log=True)[1, 0] == np.float32(np.log1p(2) / np.log1p(8))
    assert D.image(np.zeros((3, 2), dtype=np.int64)).tolist() == [[0.0, 0.0], [0.0, 0.0]]
    with pytest.raises(D.KsaError):
        D.image(counts, normalize="row")


# ------------------------------------------------------------------------------------------ command line
def test_density_key_parses(K):
    d = K.handle_args({}, ["zeroSpan", "fftSize", "512", "density", "64:-120:0", "densitySave", "/tmp/x.npy"])
    assert d["density.spec"] == (64, -120.0, 0.0) and d["densitySave"] == "/tmp/x.npy"
    d = K.handle_args({}, ["zeroSpan", "fftSize", "512"])
    assert d["density"] == "" and d["densitySave"] == "" and d["density.spec"] is None


@pytest.mark.parametrize("value", ["0:-1:0", "64:0:0", "x", "1025:-1:0", "64:-1", "64:nan:0", "6.5:-1:0"])
def test_density_key_refuses_with_the_rule(K, value, capsys):
    d = {}
    with pytest.raises(SystemExit):
        K.handle_args(d, ["zeroSpan", "fftSize", "512", "density", value])
    assert d["cmd.stop"] is True
    assert K.DENSITY_RULE in capsys.readouterr().out


def test_density_is_zerospan_only(K, capsys):
    for mode in (["scan", "startFreq", "100e6", "endFreq", "104.8e6"], ["fmScan"], ["quickFullScan"], ["zeroSpanSave"]):
        with pytest.raises(SystemExit):
            K.handle_args({}, mode + ["density", "64:-120:0"])
        assert "zeroSpan only" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        K.handle_args({}, ["zeroSpan", "bUsePSD", "true", "density", "64:-120:0"])
    d = K.handle_args({}, ["zeroSpanPlay", "fftSize", "512", "density", "64:-120:0"])
    assert d["density.spec"] is None and "WARN" in capsys.readouterr().out


def test_defaults_leave_the_reference_cases_alone(K):
    cli = json.load(open(os.path.join(GOLDEN, "cli_args.json")))
    for name, case in cli.items():
        d = K.handle_args({}, case["argv"] + ["prgLoopCnt", "0"])
        for k, want in case["d"].items():
            assert d[k] == want, (name, k)
        assert d["density.spec"] is None


# ------------------------------------------------------------------------------------------ ISA
@pytest.fixture(scope="module")
def density_asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_density")
    return _kernels(_asm(os.path.join(PKG_DIR, "csrc_density", "ksd_api.hip"), str(d / "ksd_api.s")))


def test_add_kernels_use_lds_integer_adds_and_no_scratch(density_asm):
    """The four add kernels (16-byte / 4-byte loads x plain / run-combined hits): no scratch, the partial histogram takes LDS
    integer adds (ds_add_u32, no returning form), the flush is a 64-bit integer global atomic and nothing is a float atomic;
    the vector forms load 16 bytes."""
    names = [k for k in density_asm if "add_kernel<" in k]
    assert len(names) == 4, names
    for vec in ("true", "false"):
        for combine in ("true", "false"):
            body, tail = _find(density_asm, "add_kernel<%s, %s>" % (vec, combine))
            assert _resource(tail, "ScratchSize") == 0, (vec, combine)
            mix = _mix(body)
            assert mix["ds_add_u32"] >= 1, dict(mix)
            assert not [k for k in mix if k.startswith("ds_add_rtn")], "an LDS add whose result is waited for"
            assert mix["global_atomic_add_x2"] + mix["flat_atomic_add_x2"] >= 1, dict(mix)
            assert not [k for k in mix if "atomic" in k and ("f32" in k or "f64" in k or "f16" in k)], dict(mix)
            wide = mix["global_load_dwordx4"] + mix["flat_load_dwordx4"] + mix["buffer_load_dwordx4"]
            assert (wide >= 1) == (vec == "true"), (vec, dict(mix))
