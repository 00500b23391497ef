"""CPU tests of the fp32 error yardstick (precision_model.py): that the model is as accurate as a plain fp32 FFT is known to
be, that the conditions of the device tests hold (typical bins of white input, digit coverage of the impulse positions), and that
the rule `metric(x) <= MARGIN * metric(yardstick)` sees what `assert_lin` at 1e-5 does not.

The bounds on the yardstick here are sanity checks of the model (measured: rms 0.9 to 2.8 * 2^-24, max 1.1e-6, per-bin 4.1e-7);
the device tolerance is the margin over the yardstick at run time, in test_gpu_precision.py."""
import numpy as np
import pytest

import ksa_oracle as orc
import pfb_helper
import precision_model as pm
from test_gpu_parity import assert_lin

SIZES = (16, 64, 1000, 4096, 16384, 65536)
WINDOWS = ("ones", "hanning", "hamming", "kaiser")
EPS = 2.0 ** -24


def _block(n, window, mode):
    """(samples, taps, q) of one white block: two windows' worth at 50 % overlap, or two tap segments."""
    if mode == "PFB":
        return pm.white(2 * n, 11 + n), pfb_helper.prototype(n, 2, window), None
    return pm.white(2 * n, 11 + n), orc.window_table(window, n), 0.5


@pytest.mark.parametrize("mode", ["AVG", "MAX", "PSD", "PFB"])
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("n", SIZES)
def test_yardstick_is_a_plain_fp32_fft_on_white_input(n, window, mode):
    x, win, q = _block(n, window, mode)
    want, got = pm.reference(x, n, win, mode, q), pm.yardstick(x, n, win, mode, q)
    assert got.dtype == np.float32 and want.dtype == np.float64
    if mode == "PSD":
        want, got = np.sqrt(want), np.sqrt(got.astype(np.float64))
    assert pm.rms_err(got, want) < 4 * EPS, pm.rms_err(got, want) / EPS
    assert pm.max_err(got, want) < 2e-6, pm.max_err(got, want)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("n", SIZES)
def test_white_input_has_typical_bins_only(n, window):
    """The dB check leaves out the bins under 0.1 * rms; they must be few."""
    x, win, q = _block(n, window, "AVG")
    share = np.mean(pm.typical_bins(pm.reference(x, n, win, "AVG", q)))
    assert share >= pm.SHARE, share


@pytest.mark.parametrize("mode,q", [("AVG", 0.25), ("MAX", 0.25), ("AVG", 1.0), ("PFB", None)])
@pytest.mark.parametrize("n", SIZES)
def test_yardstick_on_impulses_bin_by_bin(n, mode, q):
    """Every frame's spectrum is exactly flat in float64 and the model keeps every bin to 1e-6 of itself."""
    pos = pm.impulse_positions(n)
    if n > 4096:
        pos = pos[::7] + pos[-2:]
    win = pfb_helper.prototype(n, 2, "hamming") if mode == "PFB" else orc.window_table("kaiser", n)
    worst = 0.0
    for fr in pm.impulses(len(pos), 2 * n, pos):
        want = pm.reference(fr, n, win, mode, q)
        assert np.ptp(want) <= 1e-12 * np.max(want) and np.max(want) > 0
        worst = max(worst, pm.bin_err(pm.yardstick(fr, n, win, mode, q), want))
    assert worst < 1e-6, worst


def test_db_form_of_the_yardstick():
    n, gain = 4096, 19.1
    x, win, q = _block(n, "hanning", "AVG")
    want = pm.reference(x, n, win, "AVG", q)
    got = pm.to_db(pm.yardstick(x, n, win, "AVG", q), gain)
    assert got.dtype == np.float32
    assert np.array_equal(pm.to_db(want, gain), orc.log_no_gain(np.copy(want), gain))
    # one float32 rounding of a value near -45 dB is 1.9e-6 dB; the transform's own error adds less on a typical bin
    assert pm.db_err(got, pm.to_db(want, gain), pm.typical_bins(want)) < 2e-5


# ------------------------------------------------------------------------------------------------ sensitivity
def _fails(device, model):
    ok, ratio = pm.within(device, model)
    return not ok and ratio > pm.MARGIN


@pytest.mark.parametrize("n", [4096, 65536])
def test_rule_sees_a_relative_perturbation_that_assert_lin_passes(n):
    """2e-6 relative Gaussian noise on every bin of the truth: thirty times the fp32 level, and inside 1e-5 of the peak."""
    for x in (pm.white(2 * n, 3), orc.synth_iq(2 * n, 3).astype(np.complex64)):
        win = orc.window_table("hanning", n)
        want, model = pm.reference(x, n, win, "AVG", 0.5), pm.yardstick(x, n, win, "AVG", 0.5)
        bad = want * (1 + 2e-6 * np.random.default_rng(5).standard_normal(n))
        assert_lin(bad, want)
        assert _fails(pm.rms_err(bad, want), pm.rms_err(model, want))
        assert _fails(pm.max_err(bad, want), pm.max_err(model, want))
        assert pm.within(pm.rms_err(model, want), pm.rms_err(model, want))[0]


@pytest.mark.parametrize("n", [64, 1000, 4096])
def test_impulse_rule_sees_one_bin_off_by_3e_6(n):
    win = orc.window_table("hamming", n)
    fr = pm.impulses(1, 2 * n, [n // 3])[0]
    want, model = pm.reference(fr, n, win, "MAX", 0.25), pm.yardstick(fr, n, win, "MAX", 0.25)
    bad = want.copy()
    bad[n // 5] *= 1 + 3e-6
    assert_lin(bad, want)
    assert _fails(pm.bin_err(bad, want), pm.bin_err(model, want))


@pytest.mark.parametrize("window", ["hanning", "hamming", "kaiser"])
@pytest.mark.parametrize("n", [64, 4096])
def test_rule_sees_window_taps_rounded_to_float16(n, window):
    x, win, q = _block(n, window, "AVG")
    want, model = pm.reference(x, n, win, "AVG", q), pm.yardstick(x, n, win, "AVG", q)
    bad = pm.reference(x, n, win.astype(np.float16).astype(np.float64), "AVG", q)
    assert _fails(pm.rms_err(bad, want), pm.rms_err(model, want))


def test_floor_metric_sees_a_floor_at_minus_100_dbc():
    """The kaiser tone: the truth away from the main lobe (-174 dBc: the complex64 rounding of the input samples) is far below
    fp32 resolution, the model's floor is near -144 dBc, and a spur at -100 dBc fails both floor figures."""
    n = 4096
    x, win = pm.tone(2 * n), orc.window_table("kaiser", n)
    want, model = pm.reference(x, n, win, "AVG", 0.5), pm.yardstick(x, n, win, "AVG", 0.5)
    far = pm.far_bins(want, n)
    assert np.max(want[far]) < 10 ** (-165 / 20) * np.max(want) and pm.spur(model, want, n) < 10 ** (-135 / 20)
    bad = want.copy()
    bad[np.flatnonzero(far)[100]] += 1e-5 * np.max(want)
    assert_lin(bad, want)
    assert _fails(pm.floor_err(bad, want), pm.floor_err(model, want))
    assert _fails(pm.spur(bad, want, n), pm.spur(model, want, n))


# ------------------------------------------------------------------------------------------------ impulse positions
@pytest.mark.parametrize("n", [16, 20, 32, 64, 240, 1000, 1024, 2400, 4096, 8192, 16200, 16384, 32768, 65536, 524288, 1048576])
def test_impulse_positions_cover_every_nonzero_value_of_every_digit(n):
    radices = pm.digit_radices(n)
    assert int(np.prod(radices)) == n
    pos = pm.impulse_positions(n)
    assert 1 in pos and n - 1 in pos and all(0 <= p < n for p in pos) and len(pos) <= 80
    seen = [set() for _ in radices]
    for p in pos:
        dg = pm.digits(p, radices)
        for j, d in enumerate(dg):
            seen[j].add(d)
        if n > 16384 and p not in (1, n - 1):
            assert all(dg), (p, dg)
    if n <= 16384:
        for j, r in enumerate(radices):
            assert set(range(1, r)) <= seen[j], (j, r)
        # every digit value also stands alone in one position, so that a fault of one pass is not masked by another
        weight = 1
        for r in radices:
            assert all(d * weight in pos for d in range(1, r))
            weight *= r
    else:
        assert len(pos) == 10


def test_mixed_radix_plan_order():
    """The pass order of the mixed-radix plan (fives, threes, fours, a two, the last four)."""
    assert pm.mr_radices(20) == [5, 4]
    assert pm.mr_radices(1000) == [5, 5, 5, 2, 4]
    assert pm.mr_radices(2400) == [5, 5, 3, 4, 2, 4]
    assert pm.mr_radices(16200) == [5, 5, 3, 3, 3, 3, 2, 4]
    assert pm.mr_radices(240) == [5, 3, 4, 4]


def test_generators():
    x = pm.impulses(5, 64, [3, 9])
    assert x.dtype == np.complex64 and np.count_nonzero(x) == 5 and x[2, 3] == np.complex64(pm.IMPULSE) and x[1, 9] != 0
    w = pm.white(4096, 1)
    assert w.dtype == np.complex64 and abs(np.std(w.real) - 0.25) < 0.02
    t = pm.tone(100)
    assert t.dtype == np.complex64 and np.allclose(np.abs(t), 0.9, atol=1e-6)
