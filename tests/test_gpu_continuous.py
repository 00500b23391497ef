"""The continuous key on the GPU, through the command line: the stages' stream forms (kdc_ / kch_ / kdm_ / krs_ / kcr_ /
kpl_process_dev, kcr_flush, kpl_flush) under kspecanal.main.  The libraries' own tests pin those entry points to their models;
here the glue is under test: that the blocks reach the stages back to back, that what is handed off does not depend on
frameBatch, and that it equals the libraries driven directly over the whole capture in one call each.

Unless a test says otherwise: fftSize 256 (fullSize 2048), 2.4 MS/s, iqFormat s16, 21 frames at frameBatch 8 (batches of 8, 8
and 5), a file source of 16384 settle samples plus exactly 21 blocks, plots off.  Comparisons are bit for bit unless a tolerance
is named.  Every capture and every run that several tests read is made once per module."""
import importlib

import numpy as np
import pytest

from conftest import load_pkg
import corr_model
import pulse_model as pm

pytestmark = pytest.mark.gpu

N, FULL, FRAMES, FS = 256, 2048, 21, 2.4e6
SETTLE = 16 * 1024                                           # the samples sdr_setup discards
QUIET = ["bPltLevels", "false", "bPltHeatMap", "false", "prgLoopCnt", str(FRAMES)]
COMMON = ["zeroSpan", "fftSize", str(N), "iqFormat", "s16", "window", "hanning"] + QUIET
ON = ["continuous", "true"]
FFT_KEYS = ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg", "fftHM")
CUT_FREE = ("Fft.Cur", "Fft.Max", "Fft.Min", "fftHM")        # Fft.Avg has a test of its own: its rounding follows the frames per engine call
OFF, TONE, DEV, AMP = 300e3, 1e3, 5e3, 0.5                   # the FM tone of the demodulator's command-line test


def same(a, b):
    """Bit for bit: equal type, shape and values (field by field for records; NaN equals NaN in float arrays)."""
    if not isinstance(a, np.ndarray) and not isinstance(b, np.ndarray):
        return type(a) is type(b) and a == b
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.names:
        return all(same(a[k], b[k]) for k in a.dtype.names)
    return np.array_equal(a, b, equal_nan=a.dtype.kind in "fc")


def assert_same(got, want, keys, what):
    for k in keys:
        assert same(got[k], want[k]), (what, k)


@pytest.fixture(scope="module")
def K():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")


@pytest.fixture(scope="module")
def P():
    return load_pkg()


def run(K, argv):
    K.sdr_curscan = K._gpu_curscan
    return K.main(list(argv))


def fm_capture(path, samples, fs=FS, off=OFF, dc=0j):
    """int16 I,Q [samples][2] of the FM tone (plus a DC offset), written to path."""
    t = np.arange(samples) / fs
    x = AMP * np.exp(1j * (2 * np.pi * off * t + DEV / TONE * np.sin(2 * np.pi * TONE * t))) + dc
    iq = np.empty((samples, 2), dtype=np.int16)
    iq[:, 0], iq[:, 1] = np.round(x.real * 32767), np.round(x.imag * 32767)
    iq.tofile(path)
    return iq


def tone_fit(pcm, rate, skip=16):
    """(amplitude, residual rms) of ONE least-squares sinusoid at TONE over the whole run after its first `skip` samples."""
    y = np.asarray(pcm, dtype=np.float64)[skip:]
    tt = np.arange(skip, skip + len(y)) / float(rate)
    basis = np.stack([np.cos(2 * np.pi * TONE * tt), np.sin(2 * np.pi * TONE * tt)], axis=1)
    coef = np.linalg.lstsq(basis, y, rcond=None)[0]
    return float(np.hypot(coef[0], coef[1])), float(np.sqrt(np.mean((y - basis @ coef) ** 2)))


# ------------------------------------------------------------------------------------------ 1, 2. seamless audio
@pytest.mark.parametrize("zoom,decim", [(10, 5), (3, 16)], ids=["zoom10", "zoom3_padded_reads"])
def test_the_audio_of_a_run_is_one_seamless_tone(K, tmp_path, zoom, decim):
    """zoom 10: a block is 20480 samples, a read of 32768 cut back; zoom 3: 6144 samples, a read of 8192 cut back -- without the
    reader that keeps what a read delivers beyond its block, the blocks would not be back to back and the tone would slip.  The
    capture holds exactly 21 blocks: the padded read for the last one does not fit, the run must still get all 21."""
    block_len = zoom * FULL
    fm_capture(tmp_path / "exact.s16", SETTLE + FRAMES * block_len)
    argv = COMMON + ["frameBatch", "8", "zoom", "%d:%s" % (zoom, OFF), "demod", "fm:%d" % decim]
    d = run(K, argv + ON + ["source", "file:%s" % (tmp_path / "exact.s16")])
    rate = FS / zoom / decim
    want = DEV / (FS / zoom) * K.DEMOD_PCM_SCALE
    pcm = d["demodAudio"]
    assert d["continuous"] is True and d["demodRate"] == rate and pcm.dtype == np.int16
    assert len(pcm) == -(-FRAMES * FULL // decim)
    got, rms = tone_fit(pcm, rate)
    print("continuous zoom %d: %d samples, amplitude %.3f (want %.3f), residual rms %.4f" % (zoom, len(pcm), got, want, rms))
    assert abs(got - want) <= 0.01 * want and rms < 0.02 * want, (got, want, rms)
    if zoom != 10:
        return
    # the same signal without the key: every block fits, the run does not -- the test tells the two modes apart.  A block's
    # 402 audio samples span 8.375 ms of the 13.653 ms its padded read consumes: the tone slips 0.28 cycles at every seam
    fm_capture(tmp_path / "long.s16", SETTLE + FRAMES * 32768)     # the same signal, enough of it for 21 padded block-mode reads
    b = run(K, argv + ["source", "file:%s" % (tmp_path / "long.s16")])
    assert b["continuous"] is False and len(b["demodAudio"]) == FRAMES * b["demod.spec"]["out_per_block"]
    got_b, rms_b = tone_fit(b["demodAudio"], rate)
    print("block mode zoom %d: %d samples, amplitude %.3f (want %.3f), residual rms %.4f" % (zoom, len(b["demodAudio"]), got_b, want, rms_b))
    assert abs(got_b - want) > 0.01 * want and rms_b >= 0.02 * want, (got_b, want, rms_b)


# ------------------------------------------------------------------------------------------ the captures of tests 3 to 8
# bursts of a tone by stream position (start, length): inside block 2; across the edge of blocks 3 and 4, inside a batch; across
# the edge of blocks 7 and 8, between two batches of 8; on until the last sample of the run
BURSTS = [(2 * FULL + 500, 700), (4 * FULL - 400, 900), (8 * FULL - 350, 800), (FRAMES * FULL - 400, 400)]
TEMPLATE_AT, K_TEMPL = BURSTS[0][0] + 200, 96                # the template: 96 samples from inside the first burst
PLANTED = [6 * FULL - 40, 16 * FULL - 50]                    # copies of it across a block edge and across a batch edge
BURST_TONE = 50000.0


def burst_capture():
    """int16 I,Q [SETTLE + 21 x 2048][2]: weak noise, the bursts, and the template planted twice more."""
    rng = np.random.default_rng(2026)
    n = FRAMES * FULL
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.004
    for s, ln in BURSTS:
        x[s:s + ln] += 0.5 * np.exp(2j * np.pi * BURST_TONE / FS * np.arange(ln))
    iq = np.zeros((SETTLE + n, 2), dtype=np.int16)
    iq[SETTLE:, 0], iq[SETTLE:, 1] = np.rint(x.real * 32768 * 0.5), np.rint(x.imag * 32768 * 0.5)
    body = iq[SETTLE:]
    for p in PLANTED:
        body[p:p + K_TEMPL] = body[TEMPLATE_AT:TEMPLATE_AT + K_TEMPL]
    return iq


@pytest.fixture(scope="module")
def bursts(tmp_path_factory):
    """(capture path, the int16 samples after the settle read [n][2], template path, template complex64 [96])."""
    tmp = tmp_path_factory.mktemp("bursts")
    iq = burst_capture()
    iq.tofile(tmp / "capture.s16")
    body = iq[SETTLE:]
    t = ((body[TEMPLATE_AT:TEMPLATE_AT + K_TEMPL, 0] + 1j * body[TEMPLATE_AT:TEMPLATE_AT + K_TEMPL, 1]) / 32768).astype(np.complex64)
    np.save(tmp / "template.npy", t)
    return tmp / "capture.s16", body, tmp / "template.npy", t


RAW_KEYS = ["pulses", "-20:-26:16:8", "detect", "8:8:6:maxGap=3:events=300"]


def raw_argv(bursts):
    return COMMON + ON + ["source", "file:%s" % bursts[0], "correlate", "%s:0.9:512" % bursts[2]] + RAW_KEYS


@pytest.fixture(scope="module")
def raw_runs(K, bursts):
    """pulses, correlate and detect in one continuous run over the raw blocks, at frameBatch 1, 8 and 21."""
    return {b: run(K, raw_argv(bursts) + ["frameBatch", str(b)]) for b in (1, 8, 21)}


@pytest.fixture(scope="module")
def fm(tmp_path_factory):
    """(capture path, the int16 samples after the settle read) of the FM tone with a DC offset, 21 blocks of zoom 10."""
    tmp = tmp_path_factory.mktemp("fm")
    iq = fm_capture(tmp / "fm.s16", SETTLE + FRAMES * 10 * FULL, dc=0.01 - 0.02j)
    return tmp / "fm.s16", iq[SETTLE:]


ZOOM_KEYS = ["zoom", "10:%s" % OFF, "demod", "fm:5", "detect", "8:8:6:maxGap=3:events=300"]


@pytest.fixture(scope="module")
def zoom_runs(K, fm):
    """zoom, demod and detect in one continuous run, at frameBatch 1, 8 and 21."""
    return {b: run(K, COMMON + ON + ["source", "file:%s" % fm[0], "frameBatch", str(b)] + ZOOM_KEYS) for b in (1, 8, 21)}


# ------------------------------------------------------------------------------------------ 3. the cut does not show
def test_the_cut_into_batches_does_not_show_through_the_command_line(raw_runs, zoom_runs):
    """zoom and demod read the front end, pulses and correlate the raw blocks, and the handlers refuse the two kinds beside
    each other: so the five keys go in two runs, each with detect, each at frameBatch 1, 8 and 21."""
    d = raw_runs[8]
    assert len(d["pulseEvents"]) >= 4 and len(d["corrEvents"]) >= 3 and len(d["detectEmissions"]) >= 2
    for b in (1, 21):
        assert_same(raw_runs[b], d, ("pulseEvents", "pulseTotal", "pulseActive", "corrEvents", "corrTotal", "detectEmissions")
                    + CUT_FREE, "frameBatch %d" % b)
    d = zoom_runs[8]
    assert len(d["demodAudio"]) == -(-FRAMES * FULL // 5) and np.any(d["demodAudio"] != 0) and len(d["detectEmissions"]) >= 2
    for b in (1, 21):
        assert_same(zoom_runs[b], d, ("demodAudio", "demodRate", "detectEmissions") + CUT_FREE, "frameBatch %d" % b)
    for runs in (raw_runs, zoom_runs):
        assert all(np.all(np.isfinite(runs[8][k])) and len(runs[8][k]) > 0 for k in FFT_KEYS)


def test_the_average_curve_does_not_depend_on_the_batch_size(raw_runs, zoom_runs):
    """Fft.Avg of the same runs, bit for bit at frameBatch 1, 8 and 21, as the other curves above.  The engine folds the
    average of one call in closed form, whose float32 rounding depends on the frames per call (in block mode Fft.Avg differs
    between frameBatch 1 and 8 in the last place); a continuous run feeds it one frame per call, the reference's recursion."""
    worst = 0.0
    for name, runs in (("raw", raw_runs), ("zoom", zoom_runs)):
        for b in (1, 21):
            diff = np.abs(runs[b]["Fft.Avg"] - runs[8]["Fft.Avg"])
            worst = max(worst, float(diff.max()))
            print("Fft.Avg %s frameBatch %d against 8: %d of %d bins differ, worst %.3e dB" % (name, b, np.count_nonzero(diff), diff.size, diff.max()))
    for runs in (raw_runs, zoom_runs):
        for b in (1, 21):
            assert_same(runs[b], runs[8], ("Fft.Avg",), "frameBatch %d" % b)


# ------------------------------------------------------------------------------------------ 4. against the libraries
def engine_arrays(K, argv, zoomed):
    """What a SpectrumEngine of the command line's geometry makes of [21][fullSize] complex64 frames through frames_dev, one
    frame per call: the reference's frame loop, whose average is the recursion (a + x) / 2 per frame (the engine folds the
    average of a longer call in closed form, with another rounding)."""
    import torch
    d = K.handle_args({}, argv)
    x = np.ascontiguousarray(zoomed, dtype=np.complex64).reshape(FRAMES, d["fullSize"])
    eng = K.get_engine(d, max_frames=1)
    try:
        eng.reset()
        eng.set_flags(True, True, True)
        dev = torch.view_as_real(torch.from_numpy(x)).to("cuda:%d" % d["device"])
        for f in range(FRAMES):
            eng.frames_dev(dev[f:f + 1], K.FMT_C64, 1)
        eng.synchronize()
        K._materialize(d, eng)
    finally:
        eng.close()
        d["ksa.engine"] = None
    return d


def direct_zoom(P, K, d, raw, fmt=None):
    """DownConverter.process over the whole capture, one host call, with the command line's filter and tuning."""
    z = d["zoom.spec"]
    ddc = P.ddc.DownConverter(K.FMT_S16 if fmt is None else fmt, z["decim"], P.ddc.ddc_lowpass(z["decim"], z["taps_per_phase"]),
                              freq=z["offset"], sampling_rate=d["samplingRate"], max_in=len(raw) // 2 if fmt is None else len(raw))
    try:
        return ddc.process(raw)
    finally:
        ddc.close()


def direct_audio(P, K, d, zoomed):
    """Demodulator.process, then Resampler.process under audioRate: one host call each over the whole run."""
    s, r = d["demod.spec"], d["resample.spec"]
    front = d["zoom.spec"] if d["zoom.spec"] is not None else d["chan.spec"]
    taps = P.demod.demod_taps(s["decim"], s["taps_per_phase"], deemph_us=s["deemph_us"],
                              sampling_rate=d["samplingRate"] / front["decim"] if s["deemph_us"] is not None else None,
                              dc_block=s["mode"] == "am")
    dem = P.demod.Demodulator(s["mode"], s["decim"], taps, out_fmt="s16" if r is None else "f32", pcm_scale=K.DEMOD_PCM_SCALE,
                              max_in=len(zoomed))
    try:
        audio = dem.process(zoomed)
    finally:
        dem.close()
    if r is None:
        return audio
    res = P.resamp.Resampler(r["L"], r["M"], P.resamp.resample_taps(r["L"], r["M"], r["taps_per_phase"]), type="f32", out_fmt="s16",
                             pcm_scale=K.DEMOD_PCM_SCALE, max_in=len(audio))
    try:
        return res.process(audio)
    finally:
        res.close()


def test_zoom_and_demod_equal_the_libraries_driven_directly(K, P, fm, zoom_runs):
    d = zoom_runs[8]
    zoomed = direct_zoom(P, K, d, fm[1].reshape(-1))
    assert len(zoomed) == FRAMES * FULL
    audio = direct_audio(P, K, d, zoomed)
    assert len(audio) > 0 and same(d["demodAudio"], audio)
    argv = COMMON + ON + ["frameBatch", "8"] + ZOOM_KEYS
    assert_same(d, engine_arrays(K, argv, zoomed), FFT_KEYS, "engine over the directly zoomed frames")


def test_the_resampled_audio_equals_the_libraries_driven_directly(K, P, tmp_path):
    """2.048 MS/s, zoom 8, demod fm:1, audioRate 48000: 256 kHz -> 48 kHz is L / M = 3 / 16."""
    fs = 2048000
    argv = COMMON + ON + ["samplingRate", str(fs), "frameBatch", "8", "zoom", "8:%s" % OFF, "demod", "fm:1", "audioRate", "48000"]
    full = K.handle_args({}, argv)["fullSize"]
    iq = fm_capture(tmp_path / "fm.s16", SETTLE + FRAMES * 8 * full, fs=fs)
    d = run(K, argv + ["source", "file:%s" % (tmp_path / "fm.s16")])
    r = d["resample.spec"]
    assert (r["L"], r["M"]) == (3, 16) and d["demodRate"] == 48000
    assert len(d["demodAudio"]) == -(-FRAMES * full * 3 // 16)
    zoomed = direct_zoom(P, K, d, iq[SETTLE:].reshape(-1))
    assert same(d["demodAudio"], direct_audio(P, K, d, zoomed))
    got, rms = tone_fit(d["demodAudio"], 48000, skip=32)     # a third filter's start-up; the thresholds of test 1
    want = DEV / (fs / 8) * K.DEMOD_PCM_SCALE
    print("continuous audioRate: %d samples, amplitude %.3f (want %.3f), residual rms %.4f" % (len(d["demodAudio"]), got, want, rms))
    assert abs(got - want) <= 0.01 * want and rms < 0.02 * want, (got, want, rms)


# ------------------------------------------------------------------------------------------ 5. pulses
def events_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and all(np.array_equal(a[k], b[k]) for k in a.dtype.names)


def check_pulses(P, d, body, on, off):
    _, want, act = pm.detect(body, 16, on, off, 8, "s16", block=-1, flushed=True)
    ev = d["pulseEvents"]
    assert ev.dtype == P.pulse.EVENT_DTYPE and events_equal(ev, want)
    assert d["pulseTotal"] == len(want) and d["pulseActive"] == int(want["len"].sum())
    assert np.all(ev["block"] == -1)
    for s, ln in BURSTS:                                     # every burst is ONE record, wherever the block edges fall
        hit = [e for e in ev if abs(int(e["start"]) - s) <= 16 and abs(int(e["len"]) - ln) <= 32]
        assert len(hit) == 1, (s, ln, ev[["start", "len"]])
    last = ev[-1]
    assert last["flags"] & P.pulse.FLAG_OPEN_END and int(last["start"] + last["len"]) == len(body)
    assert not np.any(ev[:-1]["flags"] & P.pulse.FLAG_OPEN_END)


def test_pulses_across_block_and_batch_edges_are_one_record_each(K, P, bursts, raw_runs, tmp_path):
    d = raw_runs[8]
    check_pulses(P, d, bursts[1], P.pulse.db_to_power(-20), P.pulse.db_to_power(-26))
    save = tmp_path / "pulses.npz"
    d2 = run(K, COMMON + ON + ["source", "file:%s" % bursts[0], "frameBatch", "8", "pulses", "-20:-26:16:8", "pulsesSave", str(save)])
    assert events_equal(d2["pulseEvents"], d["pulseEvents"])
    z = np.load(save)
    assert bool(z["continuous"]) is True and events_equal(z["events"], d["pulseEvents"])
    for k, v in pm.describe(d["pulseEvents"], 16, FS, 0).items():             # from stream positions
        assert np.array_equal(z[k], v), k
    assert np.array_equal(z["toa_s"], d["pulseEvents"]["start"] / FS)


def test_relative_pulse_levels_come_from_the_first_block(K, P, bursts):
    d = run(K, COMMON + ON + ["source", "file:%s" % bursts[0], "frameBatch", "8", "pulses", "rel:20:14:16:8"])
    S0 = pm.detect(bursts[1][:FULL], 16, 1.0, 1.0, 1, "s16")[0]               # the first block's envelope, block form
    base = float(np.median(S0)) / 16 / P.pulse.POWER_UNIT
    check_pulses(P, d, bursts[1], base * 10.0 ** 2.0, base * 10.0 ** 1.4)


# ------------------------------------------------------------------------------------------ 6. correlate
def test_correlate_finds_templates_across_block_and_batch_edges(K, P, bursts, raw_runs, tmp_path):
    d, body, templ = raw_runs[8], bursts[1], bursts[3]
    corr = P.corr.Correlator(templ, threshold=0.9, guard=512, capacity=4096, max_in=len(body), fmt="s16")
    try:
        corr.process(body)
        corr.flush()
        want, total = corr.events()
    finally:
        corr.close()
    ev = d["corrEvents"]
    assert len(want) >= 3 and same(ev, want) and d["corrTotal"] == total and np.all(ev["block"] == -1)
    x = (body[:, 0] + 1j * body[:, 1]) / 32768.0
    for p in PLANTED:                                        # where the float64 definition peaks: the copy is exact there
        lo = p - 600
        rho = corr_model.definition(x[lo:p + K_TEMPL + 600], templ)[0][0]
        assert int(np.argmax(rho)) == p - lo and rho[p - lo] > 1 - 1e-9
        assert p in ev["pos"], (p, ev["pos"])
        assert p // FULL != (p + K_TEMPL - 1) // FULL         # it does straddle a block edge
    save = tmp_path / "corr.npz"
    d2 = run(K, COMMON + ON + ["source", "file:%s" % bursts[0], "frameBatch", "8", "correlate", "%s:0.9:512" % bursts[2],
                               "correlateSave", str(save)])
    z = np.load(save)
    assert same(d2["corrEvents"], ev) and bool(z["continuous"]) is True and same(z["events"], ev)
    frac = P.corr.refine(ev)
    assert np.array_equal(z["toa"], np.stack([np.full(len(ev), -1.0), frac, frac / FS], axis=1))


def test_block_mode_misses_what_straddles_an_edge(K, bursts, raw_runs):
    """The same capture without the key: a power-of-two block is one whole read, so the blocks are the same samples.  The
    template across an edge is not found and a burst across an edge is two records: the continuous tests above tell the modes
    apart."""
    argv = [a for a in raw_argv(bursts) if a not in ON]
    b = run(K, argv + ["frameBatch", "8"])
    pos = b["corrEvents"]["block"].astype(np.int64) * FULL + b["corrEvents"]["pos"]
    assert not any(p in pos for p in PLANTED)
    assert len(b["pulseEvents"]) > len(raw_runs[8]["pulseEvents"])
    # the engine sees the same blocks in either mode; Fft.Avg is left out: block mode folds 8 frames per call in closed form
    assert_same(b, raw_runs[8], CUT_FREE + ("detectEmissions",), "block mode against continuous")


# ------------------------------------------------------------------------------------------ 7. channels
def test_channels_equal_the_channelizer_driven_directly(K, P, tmp_path):
    argv = COMMON + ON + ["frameBatch", "8", "channels", "16:2:8:3", "demod", "fm:5"]
    iq = fm_capture(tmp_path / "fm.s16", SETTLE + FRAMES * 8 * FULL, off=3 * FS / 16)      # the tone sits in channel 3
    d = run(K, argv + ["source", "file:%s" % (tmp_path / "fm.s16")])
    c = d["chan.spec"]
    assert (c["first"], c["block_len"]) == (0, 8 * FULL) and len(d["demodAudio"]) == -(-FRAMES * FULL // 5)
    body = iq[SETTLE:].reshape(-1)
    bank = P.chan.Channelizer(K.FMT_S16, 16, 2, P.chan.chan_prototype(16, 8), max_in=len(body) // 2)
    try:
        y = bank.process(body)
    finally:
        bank.close()
    assert y.shape == (16, FRAMES * FULL)
    assert same(d["demodAudio"], direct_audio(P, K, d, y[3]))
    assert_same(d, engine_arrays(K, argv, y[3]), FFT_KEYS, "engine over the directly channelized frames")
    # the run adds three float64 sums per channel, the yardstick is one: each sum of n non-negative terms is within n 2^-53 of
    # the exact one, relatively, so the two differ by at most 2 n 2^-53 (n = re^2 and im^2 of every column)
    power = (y.real.astype(np.float64) ** 2 + y.imag.astype(np.float64) ** 2).sum(axis=1)
    want = 10 * np.log10(power / y.shape[1])
    rtol = 2 * (2 * y.shape[1]) * 2.0 ** -53
    got = 10.0 ** (d["channelsPower"] / 10)
    print("channels: worst relative difference of the channel powers %.3e (bound %.3e)" % (np.max(np.abs(got / (power / y.shape[1]) - 1)), rtol))
    assert np.argmax(d["channelsPower"]) == 3
    assert np.all(np.abs(d["channelsPower"] - want) <= 10 / np.log(10) * rtol + 4 * np.spacing(np.abs(want)))
    got, rms = tone_fit(d["demodAudio"], FS / 8 / 5)
    want_amp = DEV / (FS / 8) * K.DEMOD_PCM_SCALE
    print("continuous channels: amplitude %.3f (want %.3f), residual rms %.4f" % (got, want_amp, rms))
    assert abs(got - want_amp) <= 0.01 * want_amp and rms < 0.02 * want_amp


# ------------------------------------------------------------------------------------------ 8. iqfix in front
def test_iqfix_in_front_of_a_continuous_zoom(K, P, fm):
    argv = COMMON + ON + ["frameBatch", "8", "iqfix", "dc+iq", "zoom", "10:%s" % OFF]
    d = run(K, argv + ["source", "file:%s" % fm[0]])
    body = fm[1]
    fix = P.iqfix.IqCorrector("s16", max_in=len(body))
    try:
        fix.apply(body[:8 * 10 * FULL], accumulate=True)      # the first batch is measured, then every block is corrected
        sol = fix.solve("dc+iq")
        fixed = fix.apply(body)
    finally:
        fix.close()
    assert len(d["iqfix"]["batch"]) == 1 and all(np.float32(sol[k]) == d["iqfix"][k][0] for k in ("dc_i", "dc_q", "c", "d"))
    assert abs(sol["dc_i"] - 0.01) < 1e-3 and abs(sol["dc_q"] + 0.02) < 1e-3
    zoomed = direct_zoom(P, K, d, fixed, fmt=K.FMT_C64)
    assert len(zoomed) == FRAMES * FULL
    assert_same(d, engine_arrays(K, argv, zoomed), FFT_KEYS, "engine over the directly corrected and zoomed frames")
