"""The zeroSpan stages side by side on the GPU: a run with several additive keys on hands off, and saves, bit for bit what the
runs with each key alone do, and leaves the engine's own arrays as the plain run does.  fftSize 512, 21 frames at frameBatch 8:
two full batches and one of 5, the smallest run that crosses a batch boundary and ends on a short batch.  Every run is made
once per module; every compared list must be non-empty in the single-key run, so that nothing passes vacuously."""
import importlib

import numpy as np
import pytest

from conftest import load_pkg

pytestmark = pytest.mark.gpu

N, FRAMES = 512, 21
QUIET = ["bPltLevels", "false", "bPltHeatMap", "false", "prgLoopCnt", str(FRAMES)]
ENGINE_KEYS = ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg", "fftHM", "fftHMIndex")
HANDOFF = {
    "density": ("density", "densityNaN", "densityEdges", "densityRows"),
    "mask": ("maskEvents", "maskEventsTotal", "maskHits", "maskRows", "maskEventRows"),
    "detect": ("detectEmissions", "detectEmissionsTotal", "detectHits", "detectRows"),
    "track": ("trackTracks", "trackTotal", "trackComponents", "trackLabels"),
    "correlate": ("corrEvents", "corrTotal"),
    "pulses": ("pulseEvents", "pulseTotal", "pulseActive"),
}


def same(a, b):
    """Bit for bit: equal type, shape and values (field by field for records; NaN equals NaN in float arrays)."""
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
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


def assert_same_file(got, want, what):
    zg, zw = np.load(got), np.load(want)
    if isinstance(zg, np.ndarray):
        assert same(zg, zw), what
        return
    assert sorted(zg.files) == sorted(zw.files) and len(zg.files) > 0, what
    for k in zg.files:
        assert same(zg[k], zw[k]), (what, k)


@pytest.fixture(scope="module")
def K():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")


def run(K, argv):
    K.sdr_curscan = K._gpu_curscan
    return K.main(list(argv))


# ------------------------------------------------------------------------------------------ 1. row and raw stages together
RATE, TONE = 2048000, 50000.0
# (block, start, length): every burst covers the block's last windows, which the engine's halving average weighs most
BURSTS = [(0, 2000, 2000), (1, 2500, 1530), (3, 3000, 980), (10, 1000, 3050), (11, 2200, 1790), (12, 2600, 1400), (18, 3000, 1020)]
SETTLE = 16 * 1024                                           # the samples sdr_setup discards
KEYS = {                                                     # key -> (argv, save key, file name)
    "density": (["density", "64:-120:0"], "densitySave", "density.npy"),
    "mask": (["mask", "flat:-45"], "maskSave", "mask.npz"),
    "detect": (["detect", "16:2:8:mode=go:maxGap=3:events=300"], "detectSave", "detect.npz"),
    "track": (["track", "1:2"], "trackSave", "track.npz"),
    "correlate": (None, "correlateSave", "correlate.npz"),   # its argv names the template file
    "pulses": (["pulses", "-20:-26:16:8"], "pulsesSave", "pulses.npz"),
}


def burst_capture(full):
    """int16 I,Q [SETTLE + FRAMES x per_read][2], built as the pulse detector's command-line test builds its capture: weak noise
    with bursts of a tone planted in some blocks (block, start, length)."""
    per_read = int(2 ** np.ceil(np.log2(full)))              # what one block consumes of the capture
    rng = np.random.default_rng(2026)
    x = (rng.standard_normal((FRAMES, per_read)) + 1j * rng.standard_normal((FRAMES, per_read))) * 0.004
    for b, s, ln in BURSTS:
        x[b, s:s + ln] += 0.5 * np.exp(2j * np.pi * TONE / RATE * np.arange(ln))
    iq = np.zeros((SETTLE + FRAMES * per_read, 2), dtype=np.int16)
    flat = x.reshape(-1)
    iq[SETTLE:, 0], iq[SETTLE:, 1] = np.rint(flat.real * 32768 * 0.5), np.rint(flat.imag * 32768 * 0.5)
    return iq


@pytest.fixture(scope="module")
def together(K, tmp_path_factory):
    """{name: (d, directory)} for the plain run, the run with every key on and the runs with one key (track with detect)."""
    tmp = tmp_path_factory.mktemp("stages")
    common = ["zeroSpan", "fftSize", str(N), "samplingRate", str(RATE), "iqFormat", "s16", "window", "hanning", "frameBatch", "8"] + QUIET
    full = K.handle_args({}, common)["fullSize"]
    iq = burst_capture(full)
    iq.tofile(tmp / "capture.s16")
    first = iq[SETTLE + BURSTS[0][1] + 200:][:96]            # 96 samples from inside the capture's first burst
    np.save(tmp / "template.npy", ((first[:, 0] + 1j * first[:, 1]) / 32768).astype(np.complex64))
    common += ["source", "file:%s" % (tmp / "capture.s16")]
    argv = {k: list(v[0]) if v[0] else ["correlate", "%s:0.9:512" % (tmp / "template.npy")] for k, v in KEYS.items()}

    def one(name, keys):
        where = tmp / name
        where.mkdir()
        extra = []
        for k in keys:
            extra += argv[k] + [KEYS[k][1], str(where / KEYS[k][2])]
        return run(K, common + extra), where

    runs = {"plain": one("plain", []), "all": one("all", list(KEYS))}
    for k in KEYS:
        if k != "track":
            runs[k] = one(k, [k, "track"] if k == "detect" else [k])
    runs["track"] = runs["detect"]
    return runs


def test_single_key_runs_find_something(together):
    d = {k: v[0] for k, v in together.items()}
    assert d["density"]["densityRows"] == FRAMES and int(d["density"]["density"].sum()) + int(d["density"]["densityNaN"].sum()) > 0
    assert len(d["mask"]["maskEvents"]) >= 2 and d["mask"]["maskRows"] == FRAMES
    assert len(d["detect"]["detectEmissions"]) >= 2 and d["detect"]["detectRows"] == FRAMES
    assert len(d["track"]["trackTracks"]) >= 2
    assert len(d["correlate"]["corrEvents"]) >= 2
    assert len(d["pulses"]["pulseEvents"]) >= 2


@pytest.mark.parametrize("key", sorted(KEYS))
def test_every_stage_beside_the_others_equals_the_stage_alone(together, key):
    (d_all, dir_all), (d_one, dir_one) = together["all"], together[key]
    assert_same(d_all, d_one, HANDOFF[key], key)
    assert_same_file(dir_all / KEYS[key][2], dir_one / KEYS[key][2], key)


def test_stages_leave_the_engines_arrays_alone(together):
    plain = together["plain"][0]
    assert plain["fftHMIndex"] == FRAMES % 128
    for name, (d, _) in together.items():
        assert_same(d, plain, ENGINE_KEYS, name)


# ------------------------------------------------------------------------------------------ 2. the front-end chain
@pytest.fixture(scope="module")
def chain(K):
    # centred 100 kHz above the synthetic source's 92 MHz tone, so that the tone is no DC offset, which iqfix would remove
    common = ["zeroSpan", "fftSize", str(N), "window", "hanning", "source", "synth", "centerFreq", "92.1e6", "frameBatch", "8",
              "iqfix", "dc+iq", "zoom", "4"] + QUIET
    audio, rows = ["demod", "fm:4", "audioRate", "48000"], ["density", "64:-120:0", "detect", "16:2:8:mode=go:maxGap=3:events=300"]
    return {"all": run(K, common + audio + rows), "audio": run(K, common + audio), "rows": run(K, common + rows)}


def test_front_end_chain_feeds_audio_and_rows_alike(chain):
    d, audio, rows = chain["all"], chain["audio"], chain["rows"]
    assert len(audio["demodAudio"]) > 0 and np.any(audio["demodAudio"] != 0) and audio["demodRate"] == 48000
    assert_same(d, audio, ("demodAudio", "demodRate", "iqfix"), "behind iqfix and zoom")
    assert len(audio["iqfix"]["batch"]) >= 1 and same(rows["iqfix"], audio["iqfix"])
    assert rows["densityRows"] == FRAMES and len(rows["detectEmissions"]) >= 2
    assert_same(d, rows, HANDOFF["density"] + HANDOFF["detect"], "beside demod and audioRate")
    assert_same(d, rows, ENGINE_KEYS, "engine")
    assert_same(d, audio, ENGINE_KEYS, "engine")


# ------------------------------------------------------------------------------------------ 3. the channelizer chain
def test_channelizer_chain_does_not_depend_on_the_batch_size(K):
    common = ["zeroSpan", "fftSize", str(N), "window", "hanning", "source", "synth", "channels", "8:2:8:3", "demod", "am",
              "mask", "flat:-45"] + QUIET
    d8, d1 = run(K, common + ["frameBatch", "8"]), run(K, common + ["frameBatch", "1"])
    assert len(d8["demodAudio"]) > 0 and np.any(d8["demodAudio"] != 0) and d8["maskRows"] == FRAMES and d8["maskHits"].sum() > 0
    assert np.all(np.isfinite(d8["channelsPower"]))
    assert_same(d8, d1, ("channelsPower", "demodAudio", "maskHits"), "frameBatch 8 against 1")
