"""CPU tests of the Welch PSD fold (curScanCumuMode psd): the reference-run fixtures against the float64 restatement in
psd_helper.py, the host geometry against matplotlib, the front end's arguments, the header and the binding (no GPU needed)."""
import hashlib
import os
import re

import numpy as np
import pytest

import ksa_oracle as orc
import psd_helper as ph
from conftest import ROOT, golden, load_pkg

CURVES = ("cur", "max", "min", "avg")


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _rel(got, want):
    return float(np.max(np.abs(np.asarray(got) - np.asarray(want))) / np.max(np.abs(want)))


@pytest.fixture(scope="module")
def K():
    load_pkg()
    return __import__("importlib").import_module("prgs-sdr-kspecanal_amd.kspecanal")


@pytest.mark.parametrize("n", [64, 512, 2400, 4096])
def test_curscan_fixtures_equal_the_restatement(n):
    """What the reference's sdr_curscan returned under bUsePSD true is the helper's PSD to float64 rounding (bar 1e-12 of the
    strongest bin; 6e-16 observed), for every window / overlap case of the fixture; the input is synth_iq(full, seed)."""
    g = golden("psd_curscan_n%d" % n)
    x = orc.synth_iq(int(g["full"]), int(g["seed"])).astype(np.complex64)
    assert _sha(x) == str(g["iq_sha256"])
    seen = 0
    for w, q, key in ph.fixture_cases(g):
        e = _rel(ph.psd(x, n, q, orc.window_table(w, n)), g[key])
        print("N=%d %s q=%s: %.3g" % (n, w, q, e))
        assert e <= 1e-12, (n, w, q, e)
        seen += 1
    assert seen >= 2


def test_large_fixture_equals_the_restatement():
    g = golden("psd_curscan_n32768")
    n, x = int(g["fft_size"]), orc.synth_iq(int(g["full"]), int(g["seed"])).astype(np.complex64)
    assert _sha(x) == str(g["iq_sha256"])
    y = ph.psd(x, n, float(g["non_overlap"]), orc.window_table(str(g["window"]), n))
    assert float(np.max(np.abs(y[g["idx"]] - g["psd_at_idx"])) / float(g["peak"])) <= 1e-12
    assert _rel(y.reshape(256, -1).sum(axis=1), g["psd_decim"]) <= 1e-12


def test_zerospan_fixture_equals_the_restatement_through_the_oracle_state():
    g = golden("psd_zerospan_n512")
    st, x = ph.zerospan_state(g)
    assert _sha(x) == str(g["iq_sha256"])
    for k in CURVES:
        e = _rel(getattr(st, k), g[k])
        print(k, e)
        assert e <= 1e-12, (k, e)
    assert g["hm"].shape == st.hm.shape and _rel(st.hm, g["hm"]) <= 1e-12 and st.hm_index == int(g["frames"]) % 128


def test_scan_fixture_equals_the_restatement_through_the_oracle_state():
    g = golden("psd_scan_3band_n512")
    assert float(g["non_overlap"]) == 0.1 and ph.geometry(int(g["full"]), 512, 0.1)[0] == 460
    assert len(ph.geometry(int(g["full"]), 512, 0.1)[2]) == 69
    st, x = ph.scan_state(g)
    assert _sha(x) == str(g["iq_sha256"])
    for k in CURVES:
        e = _rel(getattr(st, k), g[k])
        print(k, e)
        assert e <= 1e-12, (k, e)
    assert _rel(st.hm, g["hm"]) <= 1e-12 and st.hm_index == int(g["hm_index"])


@pytest.mark.parametrize("n,full,q,window", [(512, 4096, 0.5, "hanning"), (64, 512, 0.1, "ones"), (4096, 32768, 0.1, "kaiser"),
                                             (4096, 8192, 0.25, "hamming"), (2400, 19200, 0.1, "hanning"), (1000, 8000, 0.3, "ones"),
                                             (512, 4096, 1.0, "kaiser"), (2400, 4800, 1.0, "hanning"), (64, 512, 0.37, "hamming")])
def test_geometry_functions_reproduce_matplotlib(n, full, q, window):
    """psd_window_starts / psd_mag_scale against matplotlib.mlab: the segment count of mlab.specgram and, through a float64
    sum of |FFT|^2 at those starts times that scale, mlab.psd itself (Fs = 2) -- power-of-two and fractional hops, q = 1."""
    from matplotlib import mlab
    ksa = load_pkg()
    win = orc.window_table(window, n)
    x = orc.synth_iq(full, 4000 + n).astype(np.complex64).astype(np.complex128)
    noverlap = int(n * (1 - q))
    starts = ksa.psd_window_starts(full, n, q)
    assert starts.dtype == np.int32 and np.array_equal(starts, ph.geometry(full, n, q)[2])
    spec, _, _ = mlab.specgram(x, NFFT=n, window=win, noverlap=noverlap, Fs=2)
    assert spec.shape[1] == len(starts)
    assert np.all(np.diff(starts) == n - noverlap) and starts[-1] + n <= full < starts[-1] + 2 * n - noverlap
    scale = ksa.psd_mag_scale(win, len(starts))
    assert scale == ph.scale(win, len(starts)) and ksa.psd_mag_scale(win, len(starts), fs=4.0) == pytest.approx(scale / 2, rel=1e-15)
    acc = np.zeros(n)
    for s in starts:
        acc += np.abs(np.fft.fft(x[s:s + n] * win)) ** 2
    pxx, _ = mlab.psd(x, NFFT=n, window=win, noverlap=noverlap)
    assert _rel(np.fft.fftshift(acc * scale), pxx) <= 1e-12
    assert _rel(ph.psd(x, n, q, win), pxx) <= 1e-12


def test_fractional_hops_differ_from_the_magnitude_folds_starts():
    ksa = load_pkg()
    a, b = ksa.psd_window_starts(32768, 4096, 0.1), ksa.window_starts(32768, 4096, 0.1)
    assert set(np.diff(a)) == {410} and set(np.diff(b)) == {409, 410}


def test_geometry_refuses_what_matplotlib_refuses():
    """noverlap must lie in [0, NFFT): nonOverlap above 1 (negative noverlap) or 0 (noverlap = NFFT) has no segments."""
    ksa = load_pkg()
    for q in (1.5, 0.0, -0.25):
        with pytest.raises(ksa.KsaError, match="no PSD segment"):
            ksa.psd_window_starts(4096, 512, q)
    with pytest.raises(ksa.KsaError, match="no PSD segment"):
        ksa.psd_window_starts(256, 512, 0.5)


def test_handle_args_accepts_psd(K):
    d = K.handle_args({}, ["zeroSpan", "curScanCumuMode", "psd"])
    assert d["curScanCumuMode"] == "PSD" and d["bUsePSD"] is False
    for mode in (["zeroSpanSave"], ["scan", "startFreq", "100e6", "endFreq", "107.2e6"], ["fmScan"], ["quickFullScan"]):
        assert K.handle_args({}, mode + ["curScanCumuMode", "PSD"])["curScanCumuMode"] == "PSD"
    d = K.handle_args({}, ["zeroSpan", "curScanCumuMode", "psd", "frameBatch", "64"])
    assert d["frameBatch"] == 64 and d["curScanCumuMode"] == "PSD"
    d = {}
    with pytest.raises(SystemExit):
        K.handle_args(d, ["zeroSpan", "curScanCumuMode", "median"])
    assert d["cmd.stop"] is True
    # bUsePSD keeps its meaning: the host diagnostic is per block, whatever the fold
    with pytest.raises(SystemExit):
        K.handle_args({}, ["zeroSpan", "curScanCumuMode", "psd", "bUsePSD", "true", "frameBatch", "64"])
    assert K.handle_args({}, ["zeroSpan", "curScanCumuMode", "psd", "bUsePSD", "true"])["bUsePSD"] is True


def test_header_and_binding():
    ksa = load_pkg()
    _lib = __import__("importlib").import_module("prgs-sdr-kspecanal_amd._lib")
    hdr = open(os.path.join(ROOT, "include", "ksa.h")).read()
    assert re.search(r"\bKSA_CUMU_PSD\s*=?\s*4\b", hdr)
    assert re.search(r"#define\s+KSA_ABI_VERSION\s+5\b", hdr) and ksa.lib.ksa_abi_version() == 5
    assert "unknown cumu_mode 4" in hdr
    assert len(_lib.SIGNATURES) == 52
    assert _lib.CUMU["PSD"] == 4 and _lib.CUMU == {"RAW": 0, "AVG": 1, "MAX": 2, "MIN": 3, "PSD": 4}
