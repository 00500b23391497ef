"""The continuous key on the CPU (no GPU, no companion library): what handle_args makes of it and where it refuses it, the
reader that hands over a source's samples back to back (sources.ContiguousReader), and the zeroSpan batch loop under the key,
driven with a stub engine and stub stages of this file's own."""
import contextlib
import importlib
import io

import numpy as np
import pytest

from conftest import load_pkg

SETTLE = 16 * 1024                                           # the samples sdr_setup discards
UNIT = 2 ** 18


@pytest.fixture(scope="module")
def K():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")


@pytest.fixture(scope="module")
def S():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.sources")


def args(K, argv):
    """(d or None when handle_args quit, what it printed)."""
    d, out = {}, io.StringIO()
    with contextlib.redirect_stdout(out):
        try:
            K.handle_args(d, list(argv))
        except SystemExit:
            return None, out.getvalue()
    return d, out.getvalue()


def same(a, b):
    """Equal type, shape and values, through dicts, lists and arrays."""
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return (isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape
                and np.array_equal(a, b, equal_nan=a.dtype.kind in "fc"))
    return type(a) is type(b) and a == b


# ------------------------------------------------------------------------------------------ 1. parsing and gating
BASE = ["zeroSpan", "fftSize", "256", "xRes", "256"]


def test_the_key_parses_as_a_boolean_and_defaults_to_false(K):
    assert args(K, BASE)[0]["continuous"] is False
    assert args(K, BASE + ["continuous", "false"])[0]["continuous"] is False
    for text in ("true", "TRUE", "True"):
        assert args(K, BASE + ["CONTINUOUS", text])[0]["continuous"] is True
    d, out = args(K, BASE + ["continuous"])
    assert d is None and "Missing value" in out
    assert K._HANDLERS.index(K._handle_continuous) < K._HANDLERS.index(K._handle_zoom)
    assert not [k for k in args(K, BASE + ["continuous", "true"])[0] if k.startswith("continuous.")]     # no spec entry


@pytest.mark.parametrize("n_fft", [256, 2400])
def test_the_specs_under_the_key(K, n_fft):
    base = ["zeroSpan", "fftSize", str(n_fft)]
    full = args(K, base)[0]["fullSize"]
    assert n_fft != 256 or full == 2048
    audio = -(-full // 5)                                    # ceil(fullSize / audioDecim): the most a block can yield

    d, _ = args(K, base + ["continuous", "true", "zoom", "10:300e3", "demod", "fm:5", "audioRate", "48000"])
    off, _ = args(K, base + ["zoom", "10:300e3", "demod", "fm:5", "audioRate", "48000"])
    assert d["zoom.spec"]["block_len"] == 10 * full and off["zoom.spec"]["block_len"] == 10 * (full - 1) + 80
    assert {k: v for k, v in d["zoom.spec"].items() if k != "block_len"} == {k: v for k, v in off["zoom.spec"].items() if k != "block_len"}
    assert d["demod.spec"]["out_per_block"] == audio and off["demod.spec"]["out_per_block"] == (full - 1 - 40) // 5 + 1
    r = d["resample.spec"]
    assert (r["L"], r["M"], r["in_per_block"], r["out_per_block"]) == (1, 1, audio, audio)
    assert sorted(d["demod.spec"]) == sorted(off["demod.spec"]) and sorted(r) == sorted(off["resample.spec"])
    assert (d["startFreq"], d["endFreq"], d["fullSize"]) == (off["startFreq"], off["endFreq"], off["fullSize"])

    d, _ = args(K, base + ["continuous", "true", "channels", "16:2:8:3", "demod", "fm:5", "audioRate", "48000"])
    off, _ = args(K, base + ["channels", "16:2:8:3", "demod", "fm:5", "audioRate", "48000"])
    c = d["chan.spec"]
    assert (c["decim"], c["first"], c["block_len"]) == (8, 0, 8 * full)
    assert (off["chan.spec"]["first"], off["chan.spec"]["block_len"]) == (16, 8 * (16 + full - 1) + 1)
    assert {k: v for k, v in c.items() if k not in ("first", "block_len")} == \
           {k: v for k, v in off["chan.spec"].items() if k not in ("first", "block_len")}
    r = d["resample.spec"]                                   # 2.4 MHz / 8 / 5 = 60 kHz -> 48 kHz: L / M = 4 / 5
    assert d["demod.spec"]["out_per_block"] == audio
    assert (r["L"], r["M"], r["in_per_block"], r["out_per_block"]) == (4, 5, audio, -(-audio * 4 // 5))


def test_the_block_form_refusals_do_not_apply_to_a_stream(K):
    short = ["zeroSpan", "fftSize", "64", "xRes", "64", "zoom", "1"]           # fullSize 512
    d, out = args(K, short + ["demod", "fm:8:64"])                            # 512 taps + 1 lead > 512
    assert d is None and "demod [fm:8:64]" in out
    d, _ = args(K, short + ["demod", "fm:8:64", "continuous", "true"])
    assert d["demod.spec"]["out_per_block"] == 64
    d, out = args(K, short + ["demod", "fm:8:60", "audioRate", "30000"])      # no whole output in a block
    assert d is None and "audioRate [30000]" in out
    d, _ = args(K, short + ["demod", "fm:8:60", "audioRate", "30000", "continuous", "true"])
    r = d["resample.spec"]
    assert (r["in_per_block"], r["out_per_block"]) == (64, -(-64 * r["L"] // r["M"]))
    d, out = args(K, short[:5] + ["demod", "fm", "continuous", "true"])       # it still needs a front end
    assert d is None and "demod [fm]" in out
    big = ["zeroSpan", "fftSize", "64", "xRes", "64", "continuous", "true", "frameBatch", "1000"]
    assert args(K, big + ["zoom", "1024:0:16"])[0] is None                    # 1000 x 1024 x 512 samples exceed MAX_IN
    assert args(K, big + ["channels", "1024:1:8"])[0] is None


@pytest.mark.parametrize("mode", ["scan", "fmScan", "quickFullScan", "zeroSpanSave"])
def test_the_key_is_zero_span_only(K, mode):
    extra = ["startFreq", "88e6", "endFreq", "108e6"] if mode == "scan" else []
    d, out = args(K, [mode, "fftSize", "64"] + extra + ["continuous", "true"])
    assert d is None and "ERROR:handle_args: continuous [true] is zeroSpan only, prgMode is [" in out
    assert args(K, [mode, "fftSize", "64"] + extra + ["continuous", "false"])[0] is not None


def test_playback_ignores_the_key_and_the_psd_diagnostic_refuses_it(K):
    d, out = args(K, ["zeroSpanPlay", "fftSize", "64", "continuous", "true"])
    assert d["continuous"] is False
    assert "WARN:handle_args: continuous [true] is ignored when playing saved spectra" in out
    d, out = args(K, BASE + ["continuous", "true", "bUsePSD", "true"])
    assert d is None
    assert "ERROR:handle_args: continuous [true] needs bUsePSD false: the PSD diagnostic is per block" in out
    assert args(K, BASE + ["continuous", "false", "bUsePSD", "true"])[0] is not None


def test_print_info_names_the_key_only_when_it_is_on(K):
    def info(argv):
        d, _ = args(K, argv)
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            K.print_info(d)
        return out.getvalue()

    on = info(BASE + ["zoom", "4", "demod", "fm:4", "continuous", "true"])
    off, plain = info(BASE + ["zoom", "4", "demod", "fm:4", "continuous", "false"]), info(BASE + ["zoom", "4", "demod", "fm:4"])
    lines = [ln for ln in on.splitlines() if ln.startswith("INFO: continuous")]
    assert len(lines) == 1 and "back-to-back stream" in lines[0] and "stream forms" in lines[0]
    assert off == plain and "continuous" not in plain and "each block is demodulated on its own" in plain


def every_key_argvs(tmp):
    """Six command lines that between them carry every additive key."""
    t = np.exp(2j * np.pi * 0.1 * np.arange(48)).astype(np.complex64)
    np.save(tmp / "template.npy", t)
    np.save(tmp / "mask.npy", np.full(64, -20.0, dtype=np.float32))
    z = ["zeroSpan", "fftSize", "64", "xRes", "64"]
    return [
        z + ["source", "synth", "device", "0", "iqFormat", "s16", "frameBatch", "8", "iqfix", "dc+iq", "iqfixSave", "f.npz", "zoom", "4:100e3:16",
             "demod", "fm:4:8:75", "demodSave", "a.wav", "audioRate", "48000:4", "density", "8:-100:0", "densitySave", "d.npy",
             "detect", "8:2:6:mode=go", "detectSave", "e.npz", "track", "2:1", "trackSave", "t.npz"],
        z + ["channels", "8:2:8:3", "channelsSave", "c.npz", "demod", "am", "mask", "learn:3:6:minBins=2", "maskSave", "m.npz", "iqFormat", "u8"],
        z + ["correlate", "%s:0.75:16:events=32" % (tmp / "template.npy"), "correlateSave", "x.npz", "pulses", "rel:20:14:16:8:events=64",
             "pulsesSave", "p.npz", "mask", "file:%s" % (tmp / "mask.npy"), "iqFormat", "s8"],
        z + ["pfbTaps", "4", "pfbSpectra", "2", "window", "hanning", "density", "8:-100:0", "mask", "flat:-20:-90"],
        ["scan", "startFreq", "88e6", "endFreq", "98e6", "fftSize", "64", "xRes", "64", "scanDetect", "8:2:6:edge=2:dc=1", "scanDetectSave", "s.npz",
         "scanTrack", "2:1", "scanTrackSave", "st.npz"],
        ["zeroSpanPlay", "fftSize", "64", "xRes", "64", "zoom", "4", "detect", "8:2:6", "pulses", "-20:-26", "pfbTaps", "2", "densitySave", "d.npy"],
    ]


def test_continuous_false_changes_nothing(K, tmp_path):
    keys = set()
    for argv in every_key_argvs(tmp_path):
        keys |= {a.upper() for a in argv}
        plain, out_plain = args(K, argv)
        off, out_off = args(K, argv + ["continuous", "false"])
        assert plain is not None and out_off == out_plain
        assert list(off) == list(plain)
        for k in plain:
            assert same(off[k], plain[k]), k
    additive = list(K._KEYS)[list(K._KEYS).index("SOURCE"):]
    assert sorted(k for k in additive if k not in keys) == ["CONTINUOUS"]       # the six carry every other additive key


# ------------------------------------------------------------------------------------------ 2. the reader
class Recording:
    """A source wrapper that notes the size, in samples, of every read asked of the source."""

    def __init__(self, sdr):
        self.sdr, self.reads = sdr, []

    def read_samples(self, n):
        self.reads.append(int(n))
        return self.sdr.read_samples(n)

    def read_bytes(self, nbytes):
        self.reads.append(int(nbytes) // 2)
        return self.sdr.read_bytes(nbytes)

    def read_iq(self, n, fmt=None):
        self.reads.append(int(n))
        return self.sdr.read_iq(n, fmt)


def counting_capture(path, fmt, samples):
    """A capture whose sample n is (I, Q) = (n mod 2^15, -(n mod 2^15) - 1) in s16 and (n mod 251, n mod 241) in u8: the
    sample's own index, readable from either part."""
    n = np.arange(samples)
    iq = np.empty((samples, 2), dtype=np.int16 if fmt == "s16" else np.uint8)
    if fmt == "s16":
        iq[:, 0], iq[:, 1] = n % 2 ** 15, -(n % 2 ** 15) - 1
    else:
        iq[:, 0], iq[:, 1] = n % 251, n % 241
    iq.tofile(path)
    return iq


LENGTHS = [1536, 6144, 8192, UNIT + 1536]                   # a padded tail read, another, a power of two, across the 2^18 unit
FORMS = [("s16", "s16"), ("u8", True), ("s16", False)]       # (capture format, sdr_read's raw): raw s16, raw u8, complex64


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("fmt,raw", FORMS, ids=["s16", "u8", "c64"])
def test_reader_hands_over_a_capture_back_to_back(K, S, tmp_path, fmt, raw, length):
    blocks, batch = 5, 2                                     # batches of 2, 2 and 1, then the end of the capture
    total = SETTLE + blocks * length + length // 2          # half a block is left over
    iq = counting_capture(tmp_path / "cap.bin", fmt, total)
    src = Recording(S.FileSdr(str(tmp_path / "cap.bin"), iq_format=fmt))
    src.read_samples(SETTLE)                                 # what sdr_setup discards
    del src.reads[:]
    reader = S.ContiguousReader(src)
    dtype, per = K.raw_dtype(raw)
    out = np.zeros((batch, per * length), dtype=dtype)
    got_blocks = []
    counts = []
    for _ in range(4):
        got = reader.read_blocks(batch, length, raw, out)
        counts.append(got)
        got_blocks += [out[i].copy() for i in range(got)]
    assert counts == [2, 2, 1, 0] and reader.read_blocks(batch, length, raw, out) == 0
    body = iq[SETTLE:]
    for i, blk in enumerate(got_blocks):
        want = body[i * length:(i + 1) * length]
        if raw:
            assert blk.dtype == want.dtype and np.array_equal(blk, want.reshape(-1)), i
        else:                                                # the values of sdr_read(sdr, length, False): read_samples' unpack as complex64
            assert blk.dtype == np.complex64 and np.array_equal(blk, S.unpack(want.reshape(-1), fmt).astype(np.complex64)), i
    assert src.reads and all(n == UNIT or (n < UNIT and n & (n - 1) == 0 and n > 0) for n in src.reads), src.reads
    fresh = S.FileSdr(str(tmp_path / "cap.bin"), iq_format=fmt)               # dtype and values are sdr_read's own
    fresh.read_samples(SETTLE)
    first = K.sdr_read(fresh, length, raw)
    assert first.dtype == got_blocks[0].dtype and np.array_equal(first, got_blocks[0])


def test_reader_loses_no_block_to_the_padding_of_the_last_read(S, tmp_path):
    """21 blocks of 6144 samples and not one sample more: the padded read of 8192 that would serve the last block does not fit
    into the capture, the allowed sizes below it do."""
    iq = counting_capture(tmp_path / "cap.bin", "s16", SETTLE + 21 * 6144)
    src = Recording(S.FileSdr(str(tmp_path / "cap.bin"), iq_format="s16"))
    src.read_samples(SETTLE)
    reader = S.ContiguousReader(src)
    out = np.zeros((8, 2 * 6144), dtype=np.int16)
    counts, seen = [], []
    for _ in range(4):
        counts.append(reader.read_blocks(8, 6144, "s16", out))
        seen.append(out[:counts[-1]].copy())
    assert counts == [8, 8, 5, 0]
    assert np.array_equal(np.concatenate(seen).reshape(-1, 2), iq[SETTLE:])
    assert all(n & (n - 1) == 0 and n <= UNIT for n in src.reads)


def test_reader_wraps_round_a_looping_capture_as_the_source_does(S, tmp_path):
    iq = counting_capture(tmp_path / "cap.bin", "s16", 3 * 4096)
    reader = S.ContiguousReader(S.FileSdr(str(tmp_path / "cap.bin"), iq_format="s16", loop=True))
    out = np.zeros((5, 2 * 4096), dtype=np.int16)
    assert reader.read_blocks(5, 4096, "s16", out) == 5
    assert np.array_equal(out.reshape(5, 4096, 2), iq.reshape(3, 4096, 2)[[0, 1, 2, 0, 1]])


@pytest.mark.parametrize("length", [1536, UNIT + 1536])
def test_reader_over_the_synthetic_source_equals_one_long_read(S, length):
    """The tones are a function of the sample index alone, so without noise one long read of a second source is the yardstick.
    The noise of a read is drawn by that read, real parts before imaginary ones: with noise the second source is read in the
    pieces the reader asked for."""
    out = np.zeros((3, length), dtype=np.complex64)
    assert S.ContiguousReader(S.SyntheticSdr(seed=5, noise=0.0)).read_blocks(3, length, False, out) == 3
    assert np.array_equal(out.reshape(-1), S.SyntheticSdr(seed=5, noise=0.0).read_samples(3 * length).astype(np.complex64))
    src = Recording(S.SyntheticSdr(seed=5))
    assert S.ContiguousReader(src).read_blocks(3, length, False, out) == 3
    twin = S.SyntheticSdr(seed=5)
    pieces = np.concatenate([twin.read_samples(n) for n in src.reads]).astype(np.complex64)
    assert np.array_equal(out.reshape(-1), pieces[:3 * length]) and np.any(out.imag != 0)


# ------------------------------------------------------------------------------------------ 3. the batch loop
N, FULL, BATCH, FRAMES = 64, 1536, 8, 21
ZOOMED = 384                                                 # d["fullSize"] of the stub runs: the frames the front end hands on
FIX_PTR, FRONT_PTR = 0xF1000, 0xD0000


class Buffer:
    """Stands in for engine.PinnedBuffer."""

    def __init__(self, shape, dtype):
        self.array = np.zeros(shape, dtype)

    def close(self):
        pass


class CountingSource:
    """complex samples whose real part is their own index; it also offers read_blocks, which a continuous run must not use."""

    def __init__(self, log, samples):
        self.log, self.pos, self.samples = log, 0, samples

    def read_samples(self, n):
        if self.pos + n > self.samples:
            raise EOFError("exhausted")
        self.pos += n
        self.log.append(("read_samples", n))
        return np.arange(self.pos - n, self.pos).astype(np.complex128)

    def read_blocks(self, k, full, raw, out):
        self.log.append(("read_blocks", k))
        return 0


class StubEngine:
    hm_width = 16

    def __init__(self, log):
        self.log = log

    def reset(self):
        pass

    def set_flags(self, *flags):
        pass

    def _pinned_out(self, name, shape):
        self.log.append(("eng.pinned_out", name, shape))
        return np.zeros(shape, np.float32)

    def frames_dev(self, src, fmt, got, cur_db=None, frame_stride=None):
        self.log.append(("eng.frames_dev", src, got, None if cur_db is None else len(cur_db), frame_stride))

    def synchronize(self):
        self.log.append(("eng.synchronize",))

    def frames(self, blocks, cur_db=False):
        self.log.append(("eng.frames", len(blocks), cur_db))
        return (np.zeros((len(blocks), N), np.float32), None) if cur_db else None


class StubStage:
    def __init__(self, log, name):
        self.log, self.name = log, name

    def handoff(self, d):
        self.log.append((self.name, "handoff"))

    def close(self):
        self.log.append((self.name, "close"))


class RowStage(StubStage):
    def feed_rows(self, db):
        self.log.append((self.name, "feed_rows", len(db)))


class RawStage(StubStage):
    def feed_raw(self, blocks, got):
        self.log.append((self.name, "feed_raw", got, blocks[:got].real.astype(np.int64).copy()))


class FixStage(RawStage):
    out_ptr = FIX_PTR


class FrontStage(StubStage):
    def front(self, src, got):
        self.log.append((self.name, "front", src if isinstance(src, int) else "batch", got))
        return FRONT_PTR, None


class AudioStage(StubStage):
    def feed(self, src, got, stride):
        self.log.append((self.name, "feed", src, got, stride))


KINDS = (("density", RowStage), ("mask", RowStage), ("detect", RowStage), ("demod", AudioStage), ("zoom", FrontStage),
         ("channels", FrontStage), ("correlate", RawStage), ("pulses", RawStage), ("iqfix", FixStage))
EVERY = ("density", "mask", "detect", "demod", "zoom", "correlate", "pulses", "iqfix")


def visits(got):
    """What one batch logs between its reads and its plot refresh with every kind of stage on: the order test_cli_pipeline_host
    pins for the block mode (its device_batch), the front end's stride being None here -- and the engine taking the batch one
    frame per call, frame i at FRONT_PTR + i x 8 x fullSize bytes with row i of the batch's dB rows, so that its average does
    not depend on the batch size."""
    engine = [("eng.frames_dev", FRONT_PTR + 8 * i * ZOOMED, 1, 1, None) for i in range(got)]
    return [("iqfix", "feed_raw", got), ("zoom", "front", FIX_PTR, got), ("eng.pinned_out", "db", (got, N))] + engine + [
            ("eng.synchronize",), ("demod", "feed", FRONT_PTR, got, None),
            ("density", "feed_rows", got), ("mask", "feed_rows", got), ("detect", "feed_rows", got),
            ("correlate", "feed_raw", got), ("pulses", "feed_raw", got), ("handoff", got)]


def test_the_batch_loop_reads_back_to_back_and_keeps_its_order(K, monkeypatch):
    log = []
    monkeypatch.setattr(K._engine, "PinnedBuffer", Buffer)
    monkeypatch.setattr(K, "_handoff", lambda d, eng, freqs, new_rows=1: log.append(("handoff", new_rows)))
    d = {"sdr": CountingSource(log, 10 ** 9), "prgLoopCnt": FRAMES, "fftSize": N, "cmd.stop": False, "continuous": True, "fullSize": ZOOMED,
         "bDataMax": True, "bDataMin": True, "bDataAvg": True}
    run = K._Run(BATCH, FULL, False, K.FMT_C64, None, np.arange(N, dtype=np.float64))
    K._zero_span_batches(d, StubEngine(log), run, [cls(log, name) for name, cls in KINDS if name in EVERY])
    assert not [e for e in log if e[0] == "read_blocks"]      # the source's own read_blocks pads its reads: it is not asked
    reads = [e[1] for e in log if e[0] == "read_samples"]
    assert all(n & (n - 1) == 0 and n <= UNIT for n in reads) and FRAMES * FULL <= sum(reads) < FRAMES * FULL + 2048
    fed = {name: np.concatenate([e[3] for e in log if e[:2] == (name, "feed_raw")]) for name in ("iqfix", "correlate", "pulses")}
    for name, blocks in fed.items():                         # block i is samples [i, i + 1) x FULL of the source
        assert np.array_equal(blocks.reshape(-1), np.arange(FRAMES * FULL)), name
    order = [e[:3] if e[1:2] == ("feed_raw",) else e for e in log if e[0] != "read_samples"]
    assert order == visits(8) + visits(8) + visits(5)
    assert d["cmd.stop"] is False

    del log[:]                                               # the same loop without the key asks the source for its blocks
    d["continuous"], d["sdr"] = False, CountingSource(log, 10 ** 9)
    K._zero_span_batches(d, StubEngine(log), run, [])
    assert ("read_blocks", 8) in log and not [e for e in log if e[0] == "read_samples"]


def test_a_continuous_run_ends_on_the_last_whole_block(K, monkeypatch, capsys):
    log = []
    monkeypatch.setattr(K._engine, "PinnedBuffer", Buffer)
    monkeypatch.setattr(K, "_handoff", lambda d, eng, freqs, new_rows=1: log.append(("handoff", new_rows)))
    d = {"sdr": CountingSource(log, 13 * FULL + 100), "prgLoopCnt": FRAMES, "fftSize": N, "cmd.stop": False, "continuous": True, "fullSize": ZOOMED,
         "bDataMax": True, "bDataMin": True, "bDataAvg": True}
    run = K._Run(BATCH, FULL, False, K.FMT_C64, None, np.arange(N, dtype=np.float64))
    K._zero_span_batches(d, StubEngine(log), run, [RawStage(log, "pulses")])
    assert [e for e in log if e[0].startswith("eng.")] == [("eng.frames", 1, False)] * 13     # no front end: frame by frame from the batch
    fed = [e for e in log if e[:2] == ("pulses", "feed_raw")]
    assert [e[2] for e in fed] == [8, 5] and np.array_equal(np.concatenate([e[3] for e in fed]).reshape(-1), np.arange(13 * FULL))
    assert d["cmd.stop"] is True and capsys.readouterr().out.count("WARN:zero_span: source exhausted, stoping...") == 1


def test_zero_span_hands_off_after_the_last_feed_and_closes_every_stage_once(K, monkeypatch):
    log = []
    names = {key: name for (key, _), (name, _) in zip(K._STAGES, KINDS)}
    seen = {}

    def stub(key, cls):
        def make(d, spec, run):
            seen[names[key]] = (d["continuous"], run.block_len)
            return cls(log, names[key])
        return make

    monkeypatch.setattr(K, "_STAGES", tuple((key, stub(key, cls)) for (key, _), (_, cls) in zip(K._STAGES, KINDS)))
    monkeypatch.setattr(K._engine, "PinnedBuffer", Buffer)
    monkeypatch.setattr(K, "_handoff", lambda d, eng, freqs, new_rows=1: log.append(("handoff", new_rows)))
    monkeypatch.setattr(K, "get_engine", lambda d, max_frames=1: StubEngine(log))
    monkeypatch.setattr(K, "_materialize", lambda d, eng: {"frames": FRAMES})
    monkeypatch.setattr(K, "sdr_setup", lambda sdr, *a: (sdr, True))
    monkeypatch.setattr(K, "sdr_curscan", K._gpu_curscan)
    d = K.handle_args({}, ["zeroSpan", "fftSize", str(N), "xRes", str(N), "frameBatch", str(BATCH), "prgLoopCnt", str(FRAMES),
                           "continuous", "true", "zoom", "4"])
    assert d["continuous"] is True and d["zoom.spec"]["block_len"] == 4 * d["fullSize"]
    for key in names:
        if key != "zoom.spec":
            d[key] = {"decim": 4, "center": d["centerFreq"], "block_len": 4 * d["fullSize"]}
    d["sdr"] = CountingSource(log, 10 ** 9)
    K.zero_span(d)
    order = [name for name, _ in KINDS]
    assert seen == {name: (True, 4 * d["fullSize"]) for name in order}        # every constructor sees the key
    feeds = [i for i, e in enumerate(log) if e[1:2] in (("feed_raw",), ("front",), ("feed",), ("feed_rows",))]
    hands = [i for i, e in enumerate(log) if e[1:] == ("handoff",)]
    closes = [i for i, e in enumerate(log) if e[1:] == ("close",)]
    assert [log[i][0] for i in hands] == order and [log[i][0] for i in closes] == order[::-1]
    assert max(feeds) < min(hands) and max(hands) < min(closes)
    assert len([e for e in log if e[0] == "handoff"]) == 3   # batches of 8, 8 and 5


def test_continuous_alone_takes_the_batch_route(K, monkeypatch):
    """No stage and frameBatch 1: the reader lives in the batch loop, so that is where the run goes."""
    log = []
    monkeypatch.setattr(K._engine, "PinnedBuffer", Buffer)
    monkeypatch.setattr(K, "_handoff", lambda d, eng, freqs, new_rows=1: log.append(("handoff", new_rows)))
    monkeypatch.setattr(K, "get_engine", lambda d, max_frames=1: StubEngine(log))
    monkeypatch.setattr(K, "_materialize", lambda d, eng: {"frames": 3})
    monkeypatch.setattr(K, "sdr_setup", lambda sdr, *a: (sdr, True))
    monkeypatch.setattr(K, "sdr_curscan", K._gpu_curscan)
    d = K.handle_args({}, ["zeroSpan", "fftSize", "96", "xRes", "96", "prgLoopCnt", "3", "continuous", "true"])
    d["sdr"] = CountingSource(log, 10 ** 9)
    K.zero_span(d)
    reads = [e[1] for e in log if e[0] == "read_samples"]
    assert [e for e in log if e[0] == "eng.frames"] == [("eng.frames", 1, False)] * 3
    assert [e for e in log if e[0] == "handoff"] == [("handoff", 1)] * 3
    assert 3 * d["fullSize"] <= sum(reads) < 3 * d["fullSize"] + max(reads)
