"""The float64 model of config_model.py pinned to what the suite already pins (no GPU): on the regular geometries of the three
generators it must be the oracle's curscan (the four folds), psd_helper.psd, pfb_helper.spectrum and pfbpsd_helper.spectrum, to
float64 rounding -- and where the scale is a power of two (rectangular window) bit for bit, which holds the np.max / np.min
selection to array_equal.  Then what the model says on geometries no generator produces, from the header's sentences alone, and
the refusals of ksa_create that need no device (validate_config runs before the first HIP call)."""
import numpy as np
import pytest

import config_helper as ch
import config_model as cm
import ksa_oracle as orc
import pfb_helper as pfb
import pfbpsd_helper as pp
import psd_helper as ph

RTOL = 1e-13      # float64 rounding: the same products in another order (mag_scale folded into one factor)
FOLDS = {"RAW": cm.RAW, "AVG": cm.AVG, "MAX": cm.MAX, "MIN": cm.MIN}


def _x(total, seed):
    return orc.synth_iq(total, seed) * 0.7


@pytest.mark.parametrize("fold", sorted(FOLDS))
@pytest.mark.parametrize("n,full,q,window", [(16, 128, 0.1, "hanning"), (64, 512, 0.5, "kaiser"), (240, 1920, 0.25, "hamming"),
                                             (1024, 2048 + 5, 0.1, "hanning"), (4096, 8192, 0.5, "hamming")])
def test_fold_modes_equal_the_oracle(n, full, q, window, fold):
    x, win = _x(full, n + 1), orc.window_table(window, n)
    starts = orc.window_starts(full, n, q)
    got = cm.spectrum(x, n, starts, win, 2.0 * orc.win_adj(win) / n, FOLDS[fold])
    np.testing.assert_allclose(got, orc.curscan(x, n, q, win, fold), rtol=RTOL, atol=0)


@pytest.mark.parametrize("fold", sorted(FOLDS))
@pytest.mark.parametrize("n,full,q", [(16, 128, 0.1), (64, 512, 0.25), (1024, 8192, 0.5)])
def test_fold_modes_equal_the_oracle_bit_for_bit_under_a_power_of_two_scale(n, full, q, fold):
    """Rectangular window, N a power of two: winAdj = 1 and 2/N scale exactly, in whatever order -- array_equal, np.max / np.min
    included (the model folds before it scales, the oracle scales before it folds; the selection must be the same)."""
    x, win = _x(full, 3 * n), np.ones(n)
    got = cm.spectrum(x, n, orc.window_starts(full, n, q), win, 2.0 / n, FOLDS[fold])
    assert np.array_equal(got, orc.curscan(x, n, q, win, fold))


@pytest.mark.parametrize("n,full,q,window", [(64, 512, 0.1, "hanning"), (1000, 8000, 0.5, "hamming"), (4096, 32768 + 77, 0.25, "kaiser")])
def test_psd_equals_the_welch_helper(n, full, q, window):
    x, win = _x(full, n + 2), orc.window_table(window, n)
    starts = ph.geometry(full, n, q)[2]
    got = cm.spectrum(x, n, starts, win, ph.scale(win, len(starts)), cm.PSD)
    np.testing.assert_allclose(got, ph.psd(x, n, q, win), rtol=RTOL, atol=0)


@pytest.mark.parametrize("n,p,window", [(16, 2, "hamming"), (64, 4, "hanning"), (2400, 16, "kaiser"), (512, 3, "hamming")])
def test_pfb_equals_the_polyphase_helper(n, p, window):
    x, taps = _x(p * n, n + p), pfb.prototype(n, p, window)
    got = cm.spectrum(x, n, np.arange(p) * n, taps, pfb.scale(taps), cm.PFB)
    np.testing.assert_allclose(got, pfb.spectrum(x, n, taps), rtol=RTOL, atol=0)


@pytest.mark.parametrize("n,p,k,tail", [(16, 2, 3, 0), (64, 4, 5, 17), (512, 3, 1, 511), (2400, 16, 2, 0)])
def test_pfbpsd_equals_the_spectrometer_helper(n, p, k, tail):
    full = (p + k - 1) * n + tail
    x, taps = _x(full, n + k), pfb.prototype(n, p, "hanning")
    starts = np.arange(p) * n
    assert cm.subframes(full, n, starts) == pp.count(full, n, taps) == k
    got = cm.spectrum(x, n, starts, taps, pp.scale(taps, k), cm.PFB_PSD)
    np.testing.assert_allclose(got, pp.spectrum(x, n, taps), rtol=RTOL, atol=0)


def test_unpack_is_the_format_definitions():
    rng = np.random.default_rng(5)
    b = rng.integers(0, 256, 64, dtype=np.uint8)
    assert np.array_equal(cm.unpack(b, cm.U8), orc.unpack_u8(b))
    assert np.array_equal(cm.unpack(b, cm.U8, 127.0, 128.0), orc.unpack_u8(b, 127.0, 128.0))
    s8 = np.array([-128, 127, 0, 1], dtype=np.int8)
    assert np.array_equal(cm.unpack(s8, cm.S8), np.array([-1 + 127j / 128, 1j / 128]))
    s16 = np.array([-32768, 32767, 3, -3], dtype=np.int16)
    assert np.array_equal(cm.unpack(s16, cm.S16), np.array([-1 + 32767j / 32768, (3 - 3j) / 32768]))
    c = (rng.standard_normal(8) + 1j * rng.standard_normal(8)).astype(np.complex64)
    assert np.array_equal(cm.unpack(c, cm.C64), c.astype(np.complex128))


def test_output_modes_are_the_oracle_steps():
    n, full = 64, 512
    x, win = _x(full, 9), orc.window_table("hanning", n)
    starts, scale = orc.window_starts(full, n, 0.5), 0.37
    lin = cm.spectrum(x, n, starts, win, scale, cm.AVG)
    min_amp = float(np.median(lin))
    assert np.array_equal(cm.spectrum(x, n, starts, win, scale, cm.AVG, cm.DB, gain=7.5), orc.log_no_gain(np.copy(lin), 7.5))
    assert np.array_equal(cm.spectrum(x, n, starts, win, scale, cm.AVG, cm.DB_CLIP, gain=7.5, min_amp=min_amp),
                          orc.log_no_gain(orc.clip2minamp(np.copy(lin), min_amp), 7.5, inf_to=0))
    zero = np.zeros(full)
    assert np.all(np.isneginf(cm.spectrum(zero, n, starts, win, scale, cm.AVG, cm.DB, gain=7.5)))
    assert np.all(cm.spectrum(zero, n, starts, win, scale, cm.AVG, cm.DB_CLIP, gain=7.5, min_amp=0.0) == 0)


def test_the_headers_sentences_on_order_and_duplicates():
    """RAW is the window listed last; AVG weighs by list position (2^-(K-k), position 0: 2^-(K-1)); MAX, MIN and PSD do not see
    the order; a start listed twice is two windows."""
    n, full = 64, 700
    x = _x(full, 21)
    taps = np.random.default_rng(2).standard_normal(n)
    starts = [3, 35, 67, 99, 131]
    one = lambda s: cm.spectrum(x, n, [s], taps, 1.0, cm.RAW)
    assert np.array_equal(cm.spectrum(x, n, starts[::-1], taps, 1.0, cm.RAW), one(3))
    assert np.array_equal(cm.spectrum(x, n, [99, 3, 131, 35], taps, 1.0, cm.RAW), one(35))
    k = len(starts)
    weights = [2.0 ** -(k - 1)] + [2.0 ** -(k - i) for i in range(1, k)]
    for order in (starts, starts[::-1], [67, 3, 131, 131, 35]):
        want = sum(w * one(s) for w, s in zip(weights, order))
        np.testing.assert_allclose(cm.spectrum(x, n, order, taps, 1.0, cm.AVG), want, rtol=RTOL, atol=0)
    for mode in (cm.MAX, cm.MIN):
        assert np.array_equal(cm.spectrum(x, n, starts, taps, 1.0, mode), cm.spectrum(x, n, [99, 3, 131, 35, 67, 3], taps, 1.0, mode))
    np.testing.assert_allclose(cm.spectrum(x, n, [3, 3, 35], taps, 1.0, cm.PSD), 2 * one(3) ** 2 + one(35) ** 2, rtol=RTOL, atol=0)
    # the polyphase count comes from the LARGEST start, wherever it is listed, and ignores a ragged tail
    assert cm.subframes(64 * 7 + 13, 64, [64, 192, 0, 128]) == 4 and cm.subframes(64 * 4, 64, [192, 0]) == 1


@pytest.mark.parametrize("case", ch.REFUSALS, ids=[c[0] for c in ch.REFUSALS])
def test_create_refuses_before_it_touches_a_device(case):
    """Every check of validate_config runs before the first HIP call, so the refusals hold on a machine without a GPU: return
    code, null handle, and a text of its own that names the field and the value."""
    _, fields, words = case
    ch.assert_refused(fields, words)
    texts = {ch.create(**c[1])[1] for c in ch.REFUSALS}
    assert len(texts) == len(ch.REFUSALS), "two refusals share one text"
