"""The zeroSpan batch loop and its stage list on the CPU: _zero_span_batches and zero_span driven with a stub engine, stub
stages that log their calls, a source that hands out a fixed number of blocks and a NumPy-backed stand-in for the page-locked
buffer.  What is pinned: the order in which a batch visits the stages, what a short last batch feeds them, that the engine is
asked for dB rows only when a row stage is on, the order of the hand-off, and that every constructed stage is closed once."""
import importlib

import numpy as np
import pytest

from conftest import load_pkg

N, FULL, BATCH = 64, 512, 8
FIX_PTR, FRONT_PTR, STRIDE = 0xF1000, 0xD0000, 7


@pytest.fixture(scope="module")
def K():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")


class Buffer:
    """Stands in for engine.PinnedBuffer."""

    def __init__(self, shape, dtype):
        self.array = np.zeros(shape, dtype)

    def close(self):
        pass


class Source:
    def __init__(self, log, blocks):
        self.log, self.left = log, blocks

    def read_blocks(self, k, full, raw, out):
        got = min(k, self.left)
        self.left -= got
        self.log.append(("read", k, full))
        return got


class Engine:
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


class Stage:
    fail_on_feed = None                              # the number of the feed that raises

    def __init__(self, log, name):
        self.log, self.name, self.feeds = log, name, 0

    def _fed(self, *what):
        self.feeds += 1
        self.log.append((self.name,) + what)
        if self.feeds == self.fail_on_feed:
            raise RuntimeError(self.name)

    def handoff(self, d):
        self.log.append((self.name, "handoff"))

    def close(self):
        self.log.append((self.name, "close"))


class Rows(Stage):
    def feed_rows(self, db):
        self._fed("feed_rows", len(db))


class Raw(Stage):
    def feed_raw(self, blocks, got):
        self._fed("feed_raw", isinstance(blocks, np.ndarray), got)


class Fix(Raw):
    out_ptr = FIX_PTR


class Front(Stage):
    def front(self, src, got):
        self._fed("front", src if isinstance(src, int) else "batch", got)
        return FRONT_PTR, STRIDE


class Audio(Stage):
    def feed(self, src, got, stride):
        self._fed("feed", src, got, stride)


KINDS = (("density", Rows), ("mask", Rows), ("detect", Rows), ("demod", Audio), ("zoom", Front), ("channels", Front),
         ("correlate", Raw), ("pulses", Raw), ("iqfix", Fix))


def drive(K, monkeypatch, names, blocks, loop_cnt=21):
    """_zero_span_batches over stub stages of the given names; returns (log, d)."""
    log = []
    monkeypatch.setattr(K._engine, "PinnedBuffer", Buffer)
    monkeypatch.setattr(K, "_handoff", lambda d, eng, freqs, new_rows=1: log.append(("handoff", new_rows)))
    d = {"sdr": Source(log, blocks), "prgLoopCnt": loop_cnt, "fftSize": N, "cmd.stop": False,
         "bDataMax": True, "bDataMin": True, "bDataAvg": True}
    run = K._Run(BATCH, FULL, False, K.FMT_C64, None, np.arange(N, dtype=np.float64))
    stages = [cls(log, name) for name, cls in KINDS if name in names]
    K._zero_span_batches(d, Engine(log), run, stages)
    return log, d


def device_batch(k, got, handoff=True):
    """What one batch logs with every kind of stage on (zoom as the front end)."""
    return ([("read", k, FULL), ("iqfix", "feed_raw", True, got), ("zoom", "front", FIX_PTR, got), ("eng.pinned_out", "db", (got, N)),
             ("eng.frames_dev", FRONT_PTR, got, got, STRIDE), ("eng.synchronize",), ("demod", "feed", FRONT_PTR, got, STRIDE),
             ("density", "feed_rows", got), ("mask", "feed_rows", got), ("detect", "feed_rows", got),
             ("correlate", "feed_raw", True, got), ("pulses", "feed_raw", True, got)] + ([("handoff", got)] if handoff else []))


EVERY = ("density", "mask", "detect", "demod", "zoom", "correlate", "pulses", "iqfix")


def test_a_batch_visits_the_stages_in_order(K, monkeypatch):
    log, d = drive(K, monkeypatch, EVERY, blocks=21)
    assert log == device_batch(8, 8) + device_batch(8, 8) + device_batch(5, 5)
    assert d["cmd.stop"] is False


def test_a_source_that_runs_out_ends_the_run_on_a_short_batch(K, monkeypatch, capsys):
    log, d = drive(K, monkeypatch, EVERY, blocks=13)
    assert log == device_batch(8, 8) + device_batch(8, 5, handoff=False)       # no third batch, no plot refresh after the stop
    assert d["cmd.stop"] is True
    assert capsys.readouterr().out.count("WARN:zero_span: source exhausted, stoping...") == 1


def test_without_a_front_end_the_engine_reads_the_batch_itself(K, monkeypatch):
    log, _ = drive(K, monkeypatch, ("density", "detect", "correlate"), blocks=8, loop_cnt=8)
    assert log == [("read", 8, FULL), ("eng.frames", 8, True), ("density", "feed_rows", 8), ("detect", "feed_rows", 8),
                   ("correlate", "feed_raw", True, 8), ("handoff", 8)]
    log, _ = drive(K, monkeypatch, ("iqfix", "mask"), blocks=8, loop_cnt=8)    # the corrector's buffer is the engine's source
    assert log == [("read", 8, FULL), ("iqfix", "feed_raw", True, 8), ("eng.pinned_out", "db", (8, N)),
                   ("eng.frames_dev", FIX_PTR, 8, 8, None), ("eng.synchronize",), ("mask", "feed_rows", 8), ("handoff", 8)]


def test_no_row_stage_no_db_rows(K, monkeypatch):
    log, _ = drive(K, monkeypatch, ("pulses",), blocks=21)
    assert [e for e in log if e[0].startswith("eng.")] == [("eng.frames", 8, False), ("eng.frames", 8, False), ("eng.frames", 5, False)]
    log, _ = drive(K, monkeypatch, ("channels", "demod"), blocks=21)
    assert not [e for e in log if e[0] == "eng.pinned_out"]
    assert [e for e in log if e[0] == "eng.frames_dev"] == [("eng.frames_dev", FRONT_PTR, g, None, STRIDE) for g in (8, 8, 5)]
    log, _ = drive(K, monkeypatch, (), blocks=21)                              # frameBatch alone
    assert [e for e in log if e[0] != "read"] == [("eng.frames", 8, False), ("handoff", 8)] * 2 + [("eng.frames", 5, False), ("handoff", 5)]


# ------------------------------------------------------------------------------------------ through zero_span
def zero_span_with_stubs(K, monkeypatch, fail=None, refuse=None):
    """zero_span with every key's spec set and every stage class replaced by a stub; `fail` = (name, n): that stage's n-th feed
    raises; `refuse`: that stage's constructor raises."""
    log = []
    names = {key: name for (key, _), (name, _) in zip(K._STAGES, KINDS)}

    def stub(key, cls):
        def make(d, spec, run):
            assert spec is d[key] and run.batch == BATCH and run.block_len == 4 * FULL and run.front is d["zoom.spec"]
            if names[key] == refuse:
                raise RuntimeError(refuse)
            stage = cls(log, names[key])
            log.append((names[key], "made"))
            if fail and fail[0] == names[key]:
                stage.fail_on_feed = fail[1]
            return stage
        return make

    assert [key for key, _ in K._STAGES] == ["density.spec", "mask.spec", "detect.spec", "demod.spec", "zoom.spec", "chan.spec",
                                             "corr.spec", "pulse.spec", "iqfix.spec"]
    monkeypatch.setattr(K, "_STAGES", tuple((key, stub(key, cls)) for (key, _), (_, cls) in zip(K._STAGES, KINDS)))
    monkeypatch.setattr(K._engine, "PinnedBuffer", Buffer)
    monkeypatch.setattr(K, "_handoff", lambda d, eng, freqs, new_rows=1: log.append(("handoff", new_rows)))
    monkeypatch.setattr(K, "get_engine", lambda d, max_frames=1: Engine(log))
    monkeypatch.setattr(K, "_materialize", lambda d, eng: {"frames": 21})
    monkeypatch.setattr(K, "sdr_setup", lambda sdr, *a: (sdr, True))
    monkeypatch.setattr(K, "sdr_curscan", K._gpu_curscan)
    d = K.handle_args({}, ["zeroSpan", "fftSize", str(N), "xRes", str(N), "frameBatch", str(BATCH), "prgLoopCnt", "21"])
    for key in names:
        d[key] = {"decim": 4, "center": d["centerFreq"], "block_len": 4 * FULL}
    d["sdr"] = Source(log, 21)
    return log, d


def test_zero_span_hands_off_in_order_and_closes_in_reverse(K, monkeypatch):
    log, d = zero_span_with_stubs(K, monkeypatch)
    K.zero_span(d)
    order = [name for name, _ in KINDS]
    assert [e[0] for e in log if e[1:] == ("made",)] == order
    assert [e[0] for e in log if e[1:] == ("handoff",)] == order
    assert [e[0] for e in log if e[1:] == ("close",)] == order[::-1]
    last_feed = max(i for i, e in enumerate(log) if len(e) > 1 and str(e[1]).startswith("feed"))
    assert last_feed < log.index(("density", "handoff")) < log.index(("iqfix", "handoff")) < log.index(("iqfix", "close"))
    assert len(d["freqs"]) == N and d["freqs"][N // 2] == d["centerFreq"]


def test_every_stage_is_closed_once_when_a_row_stage_raises_in_the_third_batch(K, monkeypatch):
    log, d = zero_span_with_stubs(K, monkeypatch, fail=("mask", 3))
    with pytest.raises(RuntimeError, match="mask"):
        K.zero_span(d)
    assert log.count(("read", 8, 4 * FULL)) == 2 and log.count(("read", 5, 4 * FULL)) == 1
    assert sorted(e[0] for e in log if e[1:] == ("close",)) == sorted(name for name, _ in KINDS)
    assert not [e for e in log if e[1:] == ("handoff",)]
    assert ("detect", "feed_rows", 5) not in log and ("density", "feed_rows", 5) in log


def test_a_stage_that_cannot_be_made_closes_the_ones_before_it(K, monkeypatch):
    log, d = zero_span_with_stubs(K, monkeypatch, refuse="correlate")
    with pytest.raises(RuntimeError, match="correlate"):
        K.zero_span(d)
    made = ["density", "mask", "detect", "demod", "zoom", "channels"]
    assert [e[0] for e in log if e[1:] == ("close",)] == made[::-1] and not [e for e in log if e[0] == "read"]


def test_playback_builds_no_stage(K, monkeypatch):
    log, d = zero_span_with_stubs(K, monkeypatch)
    monkeypatch.setattr(K, "sdr_curscan", lambda d: None)          # rebound, as zero_span_play_setup does
    d["prgLoopCnt"], d["sdr"] = 0, None
    K.zero_span(d)
    assert log == [] and d["freqs"][N // 2] == d["centerFreq"]
