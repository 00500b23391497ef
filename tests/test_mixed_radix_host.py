"""CPU tests of the mixed-radix fftSize (N = 2^a*3^b*5^c, a multiple of 4, 16..16384, not a power of two): the size rule
of the front end and the engine, the CLI fix-ups at fftSize 2400 against the reference, the reference-run mr_* fixtures against
the oracle bit for bit, and the compiled kernel (no scratch memory, no device sin / cos)."""
import json
import os
import re

import numpy as np
import pytest

import ksa_oracle as orc
from conftest import golden, load_pkg, GOLDEN, ROOT

CSRC = os.path.join(ROOT, "prgs-sdr-kspecanal_amd", "csrc")
REFUSED = (1009, 750, 24000)


def _brute(n):
    if 16 <= n <= 1 << 20 and (n & (n - 1)) == 0:
        return True
    if not (16 <= n <= 16384 and n % 4 == 0):
        return False
    return all(p in (2, 3, 5) for p in range(2, n + 1) if n % p == 0 and all(p % d for d in range(2, int(p ** 0.5) + 1)))


def _mixed(limit=16384):
    return [n for n in range(16, limit + 1) if _brute(n) and n & (n - 1)]


def test_fft_size_supported_matches_a_brute_force_table():
    eng = load_pkg().engine
    got = [n for n in range(1, 20001) if eng.fft_size_supported(n)]
    want = [n for n in range(1, 20001) if _brute(n)]
    assert got == want
    mixed = _mixed()
    assert len(mixed) == 123 and mixed[0] == 20 and mixed[-1] == 16200
    for n in (96, 240, 300, 1000, 1200, 1500, 2400, 3000, 6000, 12000, 15360):
        assert n in mixed
    for n in (2 ** 20, 2 ** 21 // 2, 16, 4096):
        assert eng.fft_size_supported(n)
    for n in REFUSED + (8, 2 ** 21, 12, 18000):
        assert not eng.fft_size_supported(n)


@pytest.mark.parametrize("n", REFUSED)
def test_engine_refuses_before_the_library(n):
    """SpectrumEngine names the rule before it would call ksa_create (no GPU is touched)."""
    pkg = load_pkg()
    with pytest.raises(pkg.KsaError, match="2\\^a\\*3\\^b\\*5\\^c"):
        pkg.SpectrumEngine(n, xres=n)


def test_handle_args_zerospan_2400_matches_the_reference(capsys):
    ks = __import__("importlib").import_module("prgs-sdr-kspecanal_amd.kspecanal")
    with open(os.path.join(GOLDEN, "mr_cli_args.json")) as f:
        case = json.load(f)["zerospan_2400"]
    d = {}
    ks.handle_args(d, case["argv"])
    assert d["xRes"] == 300 == case["d"]["xRes"]
    for k, v in case["d"].items():
        assert d[k] == v, (k, d[k], v)
    assert "setting xRes to 300" in capsys.readouterr().out


@pytest.mark.parametrize("n", REFUSED)
def test_handle_args_quits_with_the_rule(n, capsys):
    ks = __import__("importlib").import_module("prgs-sdr-kspecanal_amd.kspecanal")
    d = {}
    with pytest.raises(SystemExit):
        ks.handle_args(d, ["zeroSpan", "fftSize", str(n)])
    out = capsys.readouterr().out
    assert "fftSize %d is not supported" % n in out and "2^a*3^b*5^c" in out
    assert d["cmd.stop"]


@pytest.mark.parametrize("n", [20, 96, 240, 1000, 2400])
def test_mr_curscan_fixtures_equal_the_oracle(n):
    g = golden("mr_curscan_n%d" % n)
    x, q = g["iq"], float(g["non_overlap"])
    for window in ("ones", "hanning", "hamming", "kaiser"):
        win = orc.window_table(window, n)
        for mode in ("AVG", "MAX", "MIN", "RAW"):
            assert np.array_equal(orc.curscan(x, n, q, win, mode), g["%s_%s" % (window, mode)]), (window, mode)


@pytest.mark.parametrize("n", [12000, 15360])
def test_mr_curscan_large_fixtures_equal_the_oracle(n):
    g = golden("mr_curscan_n%d" % n)
    x = orc.synth_iq(int(g["full"]), int(g["seed"])).astype(np.complex64)
    import hashlib
    assert hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest() == str(g["iq_sha256"])
    win = orc.window_table(str(g["window"]), n)
    y = orc.curscan(x, n, float(g["non_overlap"]), win, "AVG")
    ym = orc.curscan(x, n, float(g["non_overlap"]), win, "MAX")
    idx = g["idx"]
    assert np.array_equal(y[idx], g["avg_at_idx"]) and np.array_equal(ym[idx], g["max_at_idx"])
    assert np.array_equal(y.reshape(240, -1).sum(axis=1), g["avg_decim"])
    assert np.array_equal(ym.reshape(240, -1).max(axis=1), g["max_decim"])


def test_mr_zerospan_fixture_equals_the_oracle():
    g = golden("mr_zerospan_n2400")
    n, q, full, frames = int(g["fft_size"]), float(g["non_overlap"]), int(g["full"]), int(g["frames"])
    x = orc.synth_iq(full * frames, int(g["seed"])).astype(np.complex64).reshape(frames, full)
    st, _, _ = orc.zerospan_batch(x, n, q, orc.window_table(str(g["window"]), n), "AVG", float(g["gain"]), int(g["xres"]))
    for k in ("cur", "max", "min", "avg"):
        assert np.array_equal(getattr(st, k), g[k]), k
    assert int(g["xres"]) == 300 and np.array_equal(st.hm.astype(np.float32), g["hm"])


def test_mr_scan_fixture_equals_the_oracle():
    g = golden("mr_scan_3band_n2400")
    n, full, passes, steps = int(g["fft_size"]), int(g["full"]), int(g["passes"]), int(g["steps"])
    win = orc.window_table(str(g["window"]), n)
    st = orc.ScanState(n, float(g["start_freq"]), float(g["end_freq"]), float(g["sampling_rate"]), float(g["gain"]),
                       float(g["min_amp"]), int(g["xres"]), float(g["scan_non_overlap"]), base_is_raw=bool(g["base_is_raw"]))
    assert len(st.centers) == steps and n * float(g["scan_non_overlap"]) == 1200
    x = orc.synth_iq(full * steps * passes, int(g["seed"])).astype(np.complex64).reshape(passes, steps, full)
    for p in range(passes):
        st.run_pass([orc.curscan(x[p, s], n, float(g["non_overlap"]), win, "AVG") for s in range(steps)])
    for k in ("cur", "max", "min", "avg", "hm"):
        assert np.array_equal(getattr(st, k), g[k]), k
    assert st.hm_index == int(g["hm_index"])


def test_mr_fixtures_stay_small():
    sizes = {f: os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f.startswith("mr_")}
    assert max(sizes.values()) <= os.path.getsize(os.path.join(GOLDEN, "zerospan_n4096.npz"))
    assert sum(sizes.values()) <= 3.2e6


# ------------------------------------------------------------------------------------------------ the compiled kernel
@pytest.fixture(scope="module")
def mr_asm(tmp_path_factory):
    from test_isa_regression import _asm, _kernels
    d = tmp_path_factory.mktemp("isa_mr")
    return _kernels(_asm(os.path.join(CSRC, "ksa_api.hip"), str(d / "ksa_api.s")))


def test_mixed_radix_kernel_has_no_scratch_and_no_device_trig(mr_asm):
    from test_isa_regression import _resource
    hits = sorted(k for k in mr_asm if "mixed_radix_kernel<" in k)
    assert len(hits) == 2, hits           # FMT_C64 and FMT_U8
    for k in hits:
        body, tail = mr_asm[k]
        assert _resource(tail, "ScratchSize") == 0, k
        assert _resource(tail, "NumVgprs") <= 128, k
        assert not re.search(r"\b(v_sin_f32|v_cos_f32|s_swappc|s_setpc)", body), "%s calls a sin / cos routine" % k
        assert not re.search(r"(sin|cos)f?\b", " ".join(re.findall(r"\b(?:s_call|s_swappc)\S*\s+(\S+)", body))), k
