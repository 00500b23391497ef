"""CPU tests of the polyphase filter bank front end (KSA_CUMU_PFB, pfb_taps, pfbTaps): the float64 model against the oracle, the
prototype filter and what it buys (leakage), the header / binding constants, and the refusals of SpectrumEngine and the front
end -- none of which needs a GPU."""
import importlib
import os
import re

import numpy as np
import pytest

import ksa_oracle as orc
import pfb_helper as pfb
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


@pytest.mark.parametrize("mode", ["RAW", "AVG", "MAX", "MIN"])
def test_one_tap_model_is_the_oracles_curscan(mode):
    """P = 1 with a hanning table and the reference's scale: one window at 0, so every fold of the oracle returns it -- 0.0 apart."""
    n = 256
    x = orc.synth_iq(n, 99)
    win = orc.window_table("hanning", n)
    got = pfb.spectrum(x, n, win, mag_scale=2.0 * (n / np.sum(win)) / n)
    assert np.max(np.abs(got - orc.curscan(x, n, 1.0, win, mode))) == 0.0


@pytest.mark.parametrize("n,taps,window", [(64, 4, "hamming"), (64, 4, "hanning"), (20, 3, "kaiser"), (512, 16, "ones"), (16, 1, "hanning")])
def test_prototype_filter(ksa, n, taps, window):
    w = ksa.pfb_window(n, taps, window)
    assert w.dtype == np.float64 and w.shape == (taps * n,)
    assert np.allclose(w, w[::-1], rtol=0, atol=1e-15), "the prototype is symmetric"
    assert np.array_equal(w, pfb.prototype(n, taps, window))
    assert np.array_equal(ksa.pfb_window(n, taps), ksa.pfb_window(n, taps, "hamming"))
    assert pfb.scale(w) == 2.0 / np.sum(w)


def test_leakage_of_the_default_prototype():
    """N = 64, P = 4, hanning, unit complex tone on bin 16 and half way to bin 17: the on-bin peak reads 2.0 (mag_scale =
    2 / sum), and the strongest bin two or more bins from the tone is at least 70 dB below the peak (float64: -74.9 / -77.2 dB);
    the plain 64-tap hanning spectrum of the half-bin tone leaks above -35 dB there (-30.5 dB)."""
    n, taps = 64, 4
    w = pfb.prototype(n, taps, "hanning")
    t = np.arange(taps * n)
    bins = np.fft.fftshift(np.arange(n))
    bins = np.where(bins >= n // 2, bins - n, bins)
    for tone in (16.0, 16.5):
        x = np.exp(2j * np.pi * tone * t / n)
        s = pfb.spectrum(x, n, w)
        far = np.minimum(np.abs(bins - tone), n - np.abs(bins - tone)) >= 2
        if tone == 16.0:
            assert abs(20 * np.log10(np.max(s) / 2.0)) <= 0.01 and bins[np.argmax(s)] == 16
        leak = 20 * np.log10(np.max(s[far]) / np.max(s))
        assert leak <= -70.0, (tone, leak)
    win = orc.window_table("hanning", n)
    plain = orc.curscan(x[:n], n, 1.0, win, "AVG")
    assert 20 * np.log10(np.max(plain[far]) / np.max(plain)) > -35.0


def test_header_and_binding_constants(ksa):
    _lib = importlib.import_module("prgs-sdr-kspecanal_amd._lib")
    assert re.search(r"enum\s*\{\s*KSA_CUMU_PFB\s*=\s*5\s*\}", HEADER)
    assert re.search(r"#define\s+KSA_PFB_MAX_TAPS\s+16\b", HEADER)
    assert "unknown cumu_mode 5" in HEADER and "unknown cumu_mode 4" in HEADER
    assert _lib.CUMU_PFB == 5 and ksa.CUMU_PFB == 5 and "PFB" not in _lib.CUMU
    assert ksa.pfb_window is importlib.import_module("prgs-sdr-kspecanal_amd.engine").pfb_window


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s)" % name)


def test_engine_refusals_fire_before_the_library_is_called(ksa, E, monkeypatch):
    monkeypatch.setattr(E, "lib", _NoLibrary())
    for bad in (-1, 17, 100):
        with pytest.raises(ksa.KsaError, match="pfb_taps"):
            ksa.SpectrumEngine(64, pfb_taps=bad)
    for mode in ("MAX", "MIN", "RAW", "PSD"):
        with pytest.raises(ksa.KsaError, match="cumu_mode"):
            ksa.SpectrumEngine(64, pfb_taps=4, cumu_mode=mode)
    with pytest.raises(ksa.KsaError, match="taps"):
        ksa.SpectrumEngine(64, pfb_taps=4, window=np.ones(64))           # an array must hold P*N taps
    with pytest.raises(ksa.KsaError, match="fullSize"):
        ksa.SpectrumEngine(64, pfb_taps=4, full_size=128)
    with pytest.raises(ksa.KsaError, match="unknown window"):
        ksa.SpectrumEngine(64, pfb_taps=4, window="blackman")
    with pytest.raises(AssertionError, match="ksa_create"):                # a valid shape does reach the library
        ksa.SpectrumEngine(64, pfb_taps=4, window="hanning")


def test_front_end_key(K, capsys):
    d = K.handle_args({}, ["zeroSpan", "fftSize", "512"])
    assert d["pfbTaps"] == 0 and d["fullSize"] == orc.full_size(512, 2.4e6)
    d = K.handle_args({}, ["zeroSpan", "fftSize", "512", "pfbTaps", "4", "window", "hanning", "frameBatch", "8"])
    assert d["pfbTaps"] == 4 and d["fullSize"] == 2048 and d["window"] == "WIN.HANNING" and d["frameBatch"] == 8
    assert "WARN" not in capsys.readouterr().out
    K.print_info(d)
    assert "pfbTaps [4]: fullSize[2048]" in capsys.readouterr().out
    d = K.handle_args({}, ["fmScan", "PFBTAPS", "2", "fftSize", "1024"])
    assert d["prgMode"] == "SCAN" and d["fullSize"] == 2048
    capsys.readouterr()
    for extra in (["curScanNonOverlap", "0.5"], ["curScanCumuMode", "max"]):
        K.handle_args({}, ["zeroSpan", "fftSize", "512", "pfbTaps", "4"] + extra)
        out = capsys.readouterr().out
        assert out.count("WARN") == 1 and "unused with pfbTaps" in out
    d = K.handle_args({}, ["zeroSpanPlay", "fftSize", "512", "pfbTaps", "4"])
    assert d["pfbTaps"] == 0 and d["fullSize"] == orc.full_size(512, 2.4e6)
    assert "pfbTaps [4] is ignored" in capsys.readouterr().out


@pytest.mark.parametrize("extra", [["pfbTaps", "-1"], ["pfbTaps", "17"], ["pfbTaps", "4", "bUsePSD", "true"],
                                   ["pfbTaps", "4", "curScanCumuMode", "psd"]])
def test_front_end_refusals_come_before_any_source_is_opened(K, extra, monkeypatch):
    opened = []
    monkeypatch.setattr(K, "open_source", lambda d: opened.append(1))
    with pytest.raises(SystemExit):
        K.main(["zeroSpan", "fftSize", "512", "source", "synth", "bPltLevels", "false", "bPltHeatMap", "false"] + extra)
    assert not opened
