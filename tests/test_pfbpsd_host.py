"""CPU tests of the integrating polyphase spectrometer (KSA_CUMU_PFB_PSD, pfb_spectra, pfbSpectra): the float64 model against the
pinned models of the Welch fold and of the polyphase front end, its scale convention, the header / binding constants, and the
refusals of SpectrumEngine and the front end -- none of which needs a GPU."""
import importlib
import os
import re

import numpy as np
import pytest

import ksa_oracle as orc
import pfb_helper as pfb
import pfbpsd_helper as pp
import psd_helper as psd
from conftest import ROOT, load_pkg

HEADER = open(os.path.join(ROOT, "include", "ksa.h")).read()


@pytest.fixture(scope="module")
def K():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")


@pytest.fixture(scope="module")
def E():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.engine")


@pytest.mark.parametrize("n,blocks,window", [(64, 5, "hanning"), (20, 3, "kaiser"), (256, 1, "ones")])
def test_one_tap_model_is_the_welch_model_without_overlap(n, blocks, window):
    """P = 1: K = fullSize // N segments of the N-tap window at hop N -- psd_helper.psd at non-overlap 1.0, 0.0 apart."""
    x = orc.synth_iq(blocks * n + n // 2, 7)
    taps = orc.window_table(window, n)
    assert pp.count(len(x), n, taps) == blocks
    assert np.max(np.abs(pp.spectrum(x, n, taps) - psd.psd(x, n, 1.0, taps))) == 0.0


@pytest.mark.parametrize("n,p,window", [(64, 4, "hamming"), (20, 3, "hanning"), (128, 8, "kaiser")])
def test_one_spectrum_model_is_the_squared_front_end(n, p, window):
    """K = 1: scale * |FFT(fold)|^2, the square of pfb_helper.spectrum at mag_scale 1, to 1e-12 relative."""
    x = orc.synth_iq(p * n, 11)
    taps = pfb.prototype(n, p, window)
    assert pp.count(len(x), n, taps) == 1
    want = pp.scale(taps, 1) * pfb.spectrum(x, n, taps, mag_scale=1.0) ** 2
    got = pp.spectrum(x, n, taps)
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(want)


def test_white_noise_reads_one_over_fs():
    """Unit-variance complex white noise: every bin's expectation is 1 / Fs = 0.5.  N = 64, P = 4, K = 512: the mean over the bins
    averages 64 * 512 periodograms (relative sigma about 1 / 181; consecutive sub-frames share segments, which a factor of four
    on the bound covers)."""
    n, p, k = 64, 4, 512
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((p + k - 1) * n) + 1j * rng.standard_normal((p + k - 1) * n)) / np.sqrt(2.0)
    taps = pfb.prototype(n, p, "hamming")
    s = pp.spectrum(x, n, taps)
    assert pp.count(len(x), n, taps) == k
    assert abs(np.mean(s) * pp.PSD_FS - 1.0) <= 4.0 / 181.0


def test_unit_tone_on_a_bin_reads_the_coherent_gain():
    """exp(2 pi i b t / N) on bin b: every sub-frame folds to sum_k taps[k*N + n] * exp(..), whose transform at b is sum(taps);
    K of them at scale 1 / (Fs sum(taps^2) K) read sum(taps)^2 / (Fs sum(taps^2)) there."""
    n, p, k, b = 64, 4, 5, 9
    taps = pfb.prototype(n, p, "hanning")
    t = np.arange((p + k - 1) * n)
    s = pp.spectrum(np.exp(2j * np.pi * b * t / n), n, taps)
    want = np.sum(taps) ** 2 / (pp.PSD_FS * np.sum(taps * taps))
    at = n // 2 + b
    assert np.argmax(s) == at and abs(s[at] / want - 1.0) <= 1e-12


def test_a_tail_shorter_than_a_segment_is_ignored():
    n, p, k = 32, 3, 4
    taps = pfb.prototype(n, p, "hamming")
    x = orc.synth_iq((p + k) * n, 5)
    full = (p + k - 1) * n
    assert pp.count(full, n, taps) == pp.count(full + n - 1, n, taps) == k and pp.count(full + n, n, taps) == k + 1
    assert np.array_equal(pp.spectrum(x[:full], n, taps), pp.spectrum(x[:full + n - 1], n, taps))
    # generic starts: K counts from the last one
    assert pp.count(full, n, taps, starts=[5, 0, 40]) == (full - 40 - n) // n + 1


def test_header_and_binding_constants(ksa):
    _lib = importlib.import_module("prgs-sdr-kspecanal_amd._lib")
    assert re.search(r"enum\s*\{\s*KSA_CUMU_PFB_PSD\s*=\s*6\s*\}", HEADER)
    assert "unknown cumu_mode 6" in HEADER and "unknown cumu_mode 5" in HEADER
    assert re.search(r"#define\s+KSA_ABI_VERSION\s+5\b", HEADER) and _lib.ABI_VERSION == 5
    assert _lib.CUMU == {"RAW": 0, "AVG": 1, "MAX": 2, "MIN": 3, "PSD": 4}
    assert _lib.CUMU_PFB_PSD == 6 and ksa.CUMU_PFB_PSD == 6 and _lib.CUMU_PFB == 5
    assert len(_lib.SIGNATURES) == 52
    assert set(re.findall(r"\b(ksa_[a-z0-9_]+)\s*\(", HEADER)) == set(_lib.SIGNATURES)


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s)" % name)


def test_engine_refusals_fire_before_the_library_is_called(ksa, E, monkeypatch):
    monkeypatch.setattr(E, "lib", _NoLibrary())
    with pytest.raises(ksa.KsaError, match="pfb_spectra"):
        ksa.SpectrumEngine(64, pfb_spectra=4)                             # needs pfb_taps
    with pytest.raises(ksa.KsaError, match="pfb_spectra"):
        ksa.SpectrumEngine(64, pfb_taps=4, pfb_spectra=-1)
    with pytest.raises(ksa.KsaError, match="pfb_taps"):
        ksa.SpectrumEngine(64, pfb_taps=17, pfb_spectra=4)
    for mode in ("MAX", "MIN", "RAW", "PSD"):
        with pytest.raises(ksa.KsaError, match="cumu_mode"):
            ksa.SpectrumEngine(64, pfb_taps=4, pfb_spectra=4, cumu_mode=mode)
    with pytest.raises(ksa.KsaError, match=r"fullSize 512 holds 5 spectra.*pfb_spectra is 4"):
        ksa.SpectrumEngine(64, pfb_taps=4, pfb_spectra=4, full_size=512)   # (4 + 5 - 1) * 64
    with pytest.raises(ksa.KsaError, match="fullSize"):
        ksa.SpectrumEngine(64, pfb_taps=4, pfb_spectra=4, full_size=128)
    with pytest.raises(ksa.KsaError, match="taps"):
        ksa.SpectrumEngine(64, pfb_taps=4, pfb_spectra=4, window=np.ones(64))
    for shape in (dict(), dict(full_size=7 * 64), dict(full_size=7 * 64 + 63)):   # a valid shape does reach the library
        with pytest.raises(AssertionError, match="ksa_create"):
            ksa.SpectrumEngine(64, pfb_taps=4, pfb_spectra=4, **shape)


def test_engine_geometry_and_scale(ksa, E, monkeypatch):
    """What the engine hands to ksa_create: P starts at k*N, fullSize (P+K-1)*N, mode 6 and the density scale."""
    seen = {}

    class _Capture:
        def ksa_create(self, cfg, out):
            c = cfg._obj
            seen.update(mode=c.cumu_mode, full=c.full_size, nwin=c.num_windows, scale=c.mag_scale,
                        starts=[c.window_starts[i] for i in range(c.num_windows)])
            raise AssertionError("captured")

    monkeypatch.setattr(E, "lib", _Capture())
    with pytest.raises(AssertionError, match="captured"):
        ksa.SpectrumEngine(64, pfb_taps=4, pfb_spectra=6, window="hanning")
    taps = pfb.prototype(64, 4, "hanning")
    assert seen == dict(mode=6, full=9 * 64, nwin=4, scale=pp.scale(taps, 6), starts=[0, 64, 128, 192])
    with pytest.raises(AssertionError, match="captured"):
        ksa.SpectrumEngine(64, pfb_taps=4, window="hanning")              # without the argument: what it was
    assert seen == dict(mode=5, full=4 * 64, nwin=4, scale=pfb.scale(taps), starts=[0, 64, 128, 192])


def test_front_end_key(K, capsys):
    d = K.handle_args({}, ["zeroSpan", "fftSize", "512"])
    assert d["pfbSpectra"] == 0 and d["pfbTaps"] == 0 and d["fullSize"] == orc.full_size(512, 2.4e6)
    d = K.handle_args({}, ["zeroSpan", "fftSize", "512", "pfbTaps", "4"])
    assert d["pfbSpectra"] == 0 and d["fullSize"] == 2048
    d = K.handle_args({}, ["zeroSpan", "fftSize", "512", "pfbTaps", "4", "pfbSpectra", "8", "window", "hanning", "frameBatch", "8"])
    assert d["pfbTaps"] == 4 and d["pfbSpectra"] == 8 and d["fullSize"] == 11 * 512 and d["frameBatch"] == 8
    assert "WARN" not in capsys.readouterr().out
    K.print_info(d)
    out = capsys.readouterr().out
    line = [ln for ln in out.split("\n") if "pfbSpectra" in ln]
    assert len(line) == 1 and line[0].startswith("INFO:")
    assert "pfbTaps [4]" in line[0] and "pfbSpectra [8]" in line[0] and "fullSize[5632]" in line[0] and "power, density" in line[0]
    d = K.handle_args({}, ["fmScan", "PFBSPECTRA", "3", "pfbTaps", "2", "fftSize", "1024"])
    assert d["prgMode"] == "SCAN" and d["fullSize"] == 4096 and d["pfbSpectra"] == 3
    capsys.readouterr()
    for extra in (["curScanNonOverlap", "0.5"], ["curScanCumuMode", "max"]):
        K.handle_args({}, ["zeroSpan", "fftSize", "512", "pfbTaps", "4", "pfbSpectra", "8"] + extra)
        out = capsys.readouterr().out
        assert out.count("WARN") == 1 and "unused with pfbTaps" in out
    d = K.handle_args({}, ["zeroSpanPlay", "fftSize", "512", "pfbTaps", "4", "pfbSpectra", "8"])
    assert d["pfbTaps"] == 0 and d["pfbSpectra"] == 0 and d["fullSize"] == orc.full_size(512, 2.4e6)
    out = capsys.readouterr().out
    assert "pfbSpectra [8] is ignored" in out and "pfbTaps [4] is ignored" in out and out.count("WARN") == 2


@pytest.mark.parametrize("extra", [["pfbSpectra", "8"], ["pfbSpectra", "-1", "pfbTaps", "4"], ["pfbSpectra", "8", "pfbTaps", "17"],
                                   ["pfbSpectra", "8", "pfbTaps", "4", "bUsePSD", "true"],
                                   ["pfbSpectra", "8", "pfbTaps", "4", "curScanCumuMode", "psd"]])
def test_front_end_refusals_come_before_any_source_is_opened(K, extra, monkeypatch, capsys):
    opened = []
    monkeypatch.setattr(K, "open_source", lambda d: opened.append(1))
    with pytest.raises(SystemExit):
        K.main(["zeroSpan", "fftSize", "512", "source", "synth", "bPltLevels", "false", "bPltHeatMap", "false"] + extra)
    assert not opened
    assert "ERROR" in capsys.readouterr().out
