"""Transcripts of the additive zeroSpan keys (no GPU needed): for every command line of MATRIX, whether handle_args quit, what
it printed, and what it left in d['*.spec'], startFreq, endFreq and fullSize -- compared exactly with
tests/cli_key_transcripts.json.  That file was written once by `python tests/test_cli_keys_host.py --record` from commit
93c6b8c, before the handlers were folded onto their shared helpers, so it pins every message, every spec and the order of the
checks inside each handler (which decides the message a doubly wrong command line gets).  The files that `mask file:` and
`correlate` read are written here; their directory appears in the transcripts as <TMP>."""
import contextlib
import importlib
import io
import json
import os
import sys
import tempfile

import numpy as np
import pytest

from conftest import load_pkg

TRANSCRIPTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cli_key_transcripts.json")
BASE = ["zeroSpan", "fftSize", "64", "xRes", "64"]           # fullSize 512 at the default 2.4 MHz
PLAY, SCAN, PSD = ["zeroSpanPlay"], ["fmScan"], ["bUsePSD", "true"]
Z1, Z4 = ["zoom", "1"], ["zoom", "4"]
DET = ["detect", "8:2:6"]
FM = Z4 + ["demod", "fm:4"]                                  # 2.4 MHz / 4 / 4 = 150 kHz of audio
G = "{T}/corr_good.npy"


def _bad(key, texts, *more):
    return [("%s bad %s" % (key, t), list(more) + [key, t]) for t in texts]


def _modes(key, text, *more):
    """The key under playback, under scan and with bUsePSD true."""
    return [("%s %s %s" % (key, text, tag), list(more) + [key, text] + extra)
            for tag, extra in (("play", PLAY), ("scan", SCAN), ("psd", PSD))]


MATRIX = (
    # ---- density
    [("density off, save set", ["densitySave", "x.npy"]), ("density shortest", ["density", "8:-100:0"]),
     ("density save", ["density", "1024:-100.5:0.25", "densitySave", "x.npy"])]
    + _bad("density", ["8:-100", "8:-100:0:1", "x:-100:0", "8:a:0", "8:-100:b", "0:-100:0", "1025:-100:0", "8:0:0", "8:-inf:0",
                       "8:-100:nan"])
    + _modes("density", "8:-100:0")
    + [("density bad under scan", ["density", "0:-100:0"] + SCAN), ("density bad with psd", ["density", "0:-100:0"] + PSD)]
    # ---- mask
    + [("mask off, save set", ["maskSave", "x.npz"]), ("mask shortest", ["mask", "flat:-20"]),
       ("mask flat all", ["mask", "flat:-20:-90:minBins=2:events=16", "maskSave", "x.npz"]),
       ("mask flat options reversed", ["mask", "FLAT:-20:EVENTS=16:MINBINS=2"]),
       ("mask learn", ["mask", "learn:3:6"]), ("mask learn option", ["mask", "learn:3:6.5:minBins=4"]),
       ("mask file one line", ["mask", "file:{T}/mask_one.npy"]), ("mask file two lines", ["mask", "file:{T}/mask_two.npy:events=8"])]
    + _bad("mask", ["flat", "flat:1:2:3", "flat:x", "flat:-90:-20", "flat:nan", "cone:1", "learn:3", "learn:0:6", "learn:3:inf",
                    "learn:x:6", "learn:3:6:7", "file:", "flat:-20:minBins=0", "flat:-20:minBins=65", "flat:-20:events=0",
                    "flat:-20:events=1048577", "flat:-20:bogus=3", "flat:-20:minBins", "flat:-20:minBins=2:minBins=3",
                    "flat:-20:minBins=x", "file:{T}/mask_missing.npy", "file:{T}/mask_shape.npy", "file:{T}/mask_nan.npy",
                    "file:{T}/mask_crossed.npy"])
    + _modes("mask", "flat:-20")
    + [("mask missing file under scan", ["mask", "file:{T}/mask_missing.npy"] + SCAN),
       ("mask bad under play", ["mask", "flat:x"] + PLAY), ("mask bad with psd", ["mask", "flat:x"] + PSD)]
    # ---- zoom
    + [("zoom shortest", Z4), ("zoom all", ["zoom", "4:100e3:16"]), ("zoom negative offset", ["zoom", "1024:-1.2e6:1"])]
    + _bad("zoom", ["4:1:2:3", "x", "0", "1025", "4:nan", "4:1.3e6", "4:y", "4:0:0", "4:0:17", "4:0:z"])
    + _modes("zoom", "4")
    + [("zoom batch limit", ["zoom", "1024:0:16", "frameBatch", "1000"]), ("zoom bad under scan", ["zoom", "0"] + SCAN),
       ("zoom with channels under play", Z4 + ["channels", "8"] + PLAY)]
    # ---- channels
    + [("channels off, save set", ["channelsSave", "x.npz"]), ("channels shortest", ["channels", "8"]),
       ("channels all", ["channels", "8:2:8:3", "channelsSave", "x.npz"]), ("channels critically sampled", ["channels", "16:1:4:15"])]
    + _bad("channels", ["8:2:8:3:1", "x", "1", "2048", "12", "8:3", "2:4", "8:2:0", "8:2:33", "1024:2:16", "8:2:8:8", "8:2:8:-1",
                        "8:x", "8:2:y", "8:2:8:z"])
    + _modes("channels", "8")
    + [("channels with zoom", Z4 + ["channels", "8"]), ("channels batch limit", ["channels", "1024:1:8", "frameBatch", "1000"]),
       ("channels bad with psd", ["channels", "12"] + PSD)]
    # ---- detect
    + [("detect off, save set", ["detectSave", "x.npz"]), ("detect shortest", DET),
       ("detect all", ["detect", "8:2:6.5:mode=go:minWidth=2:maxGap=1:events=64", "detectSave", "x.npz"]),
       ("detect upper case", ["detect", "8:0:0:MODE=SO:EVENTS=1"])]
    + _bad("detect", ["8:2", "x:2:6", "8:y:6", "8:2:z", "0:2:6", "1025:2:6", "8:-1:6", "8:257:6", "8:2:-1", "8:2:101", "8:2:nan",
                      "8:2:6:mode=xx", "8:2:6:minWidth=0", "8:2:6:minWidth=65", "8:2:6:maxGap=-1", "8:2:6:maxGap=1025",
                      "8:2:6:events=0", "8:2:6:events=1048577", "8:2:6:bogus=1", "8:2:6:mode", "8:2:6:mode=ca:mode=go",
                      "8:2:6:minWidth=x"])
    + _modes("detect", "8:2:6")
    + [("detect fftSize too large", ["fftSize", "32768", "detect", "8:2:6"]), ("detect bad under scan", ["detect", "8:2"] + SCAN)]
    # ---- track
    + [("track off, save set", ["trackSave", "x.npz"]), ("track shortest", DET + ["track", "2:1"]),
       ("track all", DET + ["track", "2:1:minRows=3:minSpans=2:events=64", "trackSave", "x.npz"]),
       ("track without detect", ["track", "2:1"])]
    + _bad("track", ["2", "x:1", "2:y", "-1:1", "1025:1", "2:-1", "2:65", "2:1:minRows=0", "2:1:minSpans=0", "2:1:minRows=2147483648",
                     "2:1:events=0", "2:1:events=1048577", "2:1:bogus=1", "2:1:minRows", "2:1:events=4:events=5", "2:1:minRows=x"], *DET)
    + _modes("track", "2:1")
    + [("track bad without detect", ["track", "2"])]
    # ---- demod
    + [("demod off, save set", ["demodSave", "x.wav"]), ("demod shortest", Z1 + ["demod", "am"]),
       ("demod all", Z4 + ["demod", "fm:4:8:75", "demodSave", "x.wav"]), ("demod upper case", Z1 + ["demod", "PM:2"]),
       ("demod behind channels", ["channels", "8:2:8:3", "demod", "am"]), ("demod fractional rate", ["zoom", "7", "demod", "am"]),
       ("demod without a front end", ["demod", "am"]), ("demod block too short", Z1 + ["demod", "fm:8:64"]),
       ("demod block just long enough", Z1 + ["demod", "am:8:64"])]
    + _bad("demod", ["am:1:8:75:1", "xx", "am:0", "am:257", "am:1:0", "am:256:17", "am:1:8:0", "am:1:8:inf", "am:x", "am:1:y",
                     "am:1:8:z"], *Z1)
    + _modes("demod", "am")
    + [("demod bad under scan", ["demod", "xx"] + SCAN)]
    # ---- audioRate
    + [("audioRate shortest", FM + ["audioRate", "48000"]), ("audioRate all", FM + ["audioRate", "48000:4"]),
       ("audioRate without demod", ["audioRate", "48000"]), ("audioRate ratio refused", FM + ["audioRate", "1"]),
       ("audioRate fractional input", ["zoom", "7", "demod", "am", "audioRate", "48000"]),
       ("audioRate too many taps", FM + ["audioRate", "48000:65"]),
       ("audioRate no output", Z1 + ["demod", "fm:8:60", "audioRate", "30000"])]
    + _bad("audioRate", ["48000:4:1", "x", "0", "0.5", "48000.5", "inf", "48000:0", "48000:y"], *FM)
    + _modes("audioRate", "48000")
    + [("audioRate bad under scan", ["audioRate", "x"] + SCAN)]
    # ---- correlate
    + [("correlate off, save set", ["correlateSave", "x.npz"]), ("correlate shortest", ["correlate", G]),
       ("correlate all", ["correlate", G + ":0.75:16:events=32", "correlateSave", "x.npz"]),
       ("correlate bank", ["correlate", "{T}/corr_bank.npy:1:4096:EVENTS=1048576"])]
    + _bad("correlate", ["a:b:c:d:e", ":0.5", G + ":x", G + ":0", G + ":1.5", G + ":nan", G + ":0.5:0", G + ":0.5:4097", G + ":0.5:y",
                         G + ":0.5:8:events=0", G + ":0.5:8:events=1048577", G + ":0.5:8:bogus=4", G + ":0.5:8:events",
                         G + ":0.5:8:events=x", "{T}/corr_missing.npy", "{T}/corr_shape.npy", "{T}/corr_real.npy", "{T}/corr_nan.npy",
                         "{T}/corr_zero.npy", "{T}/corr_bank_zero.npy", "{T}/corr_too_long.npy", "{T}/corr_longer_than_block.npy"])
    + _modes("correlate", G)
    + [("correlate with zoom", Z4 + ["correlate", G]), ("correlate with channels", ["channels", "8", "correlate", G]),
       ("correlate missing file under scan", ["correlate", "{T}/corr_missing.npy"] + SCAN),
       ("correlate bad text and missing file", ["correlate", "{T}/corr_missing.npy:0"])]
    # ---- pulses
    + [("pulses off, save set", ["pulsesSave", "x.npz"]), ("pulses shortest", ["pulses", "-20:-26"]),
       ("pulses all", ["pulses", "REL:20:14:16:8:events=64", "pulsesSave", "x.npz"]),
       ("pulses absolute all", ["pulses", "6:-26.5:4096:1048576:EVENTS=1"]), ("pulses beside correlate", ["correlate", G, "pulses", "-20:-26"])]
    + _bad("pulses", ["-20", "rel", "rel:20", "-20:-26:16:8:events=4:9", "x:-26", "-20:y", "-26:-20", "nan:-26", "-20:-26:0",
                      "-20:-26:4097", "-20:-26:16:0", "-20:-26:16:1048577", "-20:-26:16:8:events=0", "-20:-26:16:8:events=1048577",
                      "-20:-26:16:8:bogus=4", "-20:-26:16:8:events", "-20:-26:16:8:events=x", "7:-26", "-20:-200", "-20:-26:w"])
    + _modes("pulses", "-20:-26")
    + [("pulses with zoom", Z4 + ["pulses", "-20:-26"]), ("pulses with channels", ["channels", "8", "pulses", "-20:-26"]),
       ("pulses bad under scan", ["pulses", "-20"] + SCAN)]
    # ---- iqfix
    + [("iqfix off, save set", ["iqfixSave", "x.npz"]), ("iqfix shortest", ["iqfix", "dc"]),
       ("iqfix blocks", ["frameBatch", "4", "iqfix", "DC+IQ:blocks=2", "iqfixSave", "x.npz"]), ("iqfix track", ["iqfix", "iq:track"]), ("iqfix upper case", ["iqfix", "DC:Track"]),
       ("iqfix before zoom", Z4 + ["frameBatch", "8", "iqfix", "dc+iq:blocks=8"])]
    + _bad("iqfix", ["xx", "dc:blocks=0", "dc:blocks=2", "dc:blocks=x", "dc:blocks", "dc:track=1", "dc:track:track",
                     "dc:blocks=1:blocks=1", "dc:track:blocks=1", "dc:blocks=1:track", "dc:bogus=1", "dc:bogus"])
    + _modes("iqfix", "dc")
    + [("iqfix with channels", ["channels", "8", "iqfix", "dc"]), ("iqfix with correlate", ["correlate", G, "iqfix", "dc"]),
       ("iqfix with pulses", ["pulses", "-20:-26", "iqfix", "dc"]), ("iqfix batch limit", ["frameBatch", "600000", "iqfix", "dc"]),
       ("iqfix before the largest zoom", ["zoom", "1024:0:16", "frameBatch", "497", "iqfix", "dc"]),
       ("iqfix bad under scan", ["iqfix", "xx"] + SCAN), ("iqfix bad with psd", ["iqfix", "xx"] + PSD)]
    # ---- all of them at once
    + [("everything that goes together", ["density", "8:-100:0", "mask", "learn:3:6", "detect", "8:2:6", "track", "2:1", "correlate", G,
                                          "pulses", "rel:20:14"]),
       ("the front-end chain", ["frameBatch", "8", "iqfix", "dc+iq", "density", "8:-100:0", "detect", "8:2:6"] + FM + ["audioRate", "48000"])]
)


def write_files(tmp):
    """What `mask file:` and `correlate` read: good files and one per way a file can be wrong (the missing ones stay missing)."""
    n, rng = 64, np.random.default_rng(7)
    save = lambda name, a: np.save(os.path.join(tmp, name), a)
    save("mask_one.npy", np.linspace(-30, -20, n).astype(np.float32))
    save("mask_two.npy", np.stack([np.full(n, -20.0), np.linspace(-90, -80, n)]))
    save("mask_shape.npy", np.zeros(n + 1, dtype=np.float32))
    nan = np.zeros(n, dtype=np.float32)
    nan[5] = np.nan
    save("mask_nan.npy", nan)
    save("mask_crossed.npy", np.stack([np.full(n, -20.0), np.full(n, -10.0)]).astype(np.float32))
    t = (rng.integers(-8, 9, 48) + 1j * rng.integers(-8, 9, 48)).astype(np.complex64) / 8
    save("corr_good.npy", t)
    save("corr_bank.npy", t.reshape(2, 24).astype(np.complex128))
    save("corr_shape.npy", t.reshape(2, 2, 12))
    save("corr_real.npy", t.real.copy())
    bad = t.copy()
    bad[3] = complex(np.nan, 0)
    save("corr_nan.npy", bad)
    save("corr_zero.npy", np.zeros(16, dtype=np.complex64))
    bank = t.reshape(2, 24).copy()
    bank[1] = 0
    save("corr_bank_zero.npy", bank)
    save("corr_too_long.npy", np.ones(4097, dtype=np.complex64))
    save("corr_longer_than_block.npy", np.ones(513, dtype=np.complex64))


def _plain(v, tmp):
    if isinstance(v, dict):
        return {k: _plain(x, tmp) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x, tmp) for x in v]
    if isinstance(v, np.ndarray):
        return {"re": v.real.tolist(), "im": v.imag.tolist()} if np.iscomplexobj(v) else v.tolist()
    if isinstance(v, np.generic):
        return v.item()
    if isinstance(v, str):
        return v.replace(tmp, "<TMP>")
    return v


def transcript(K, argv, tmp):
    """(did it quit, what it printed, what it left) for one command line; `{T}` in argv is the directory of write_files."""
    d, out, exited = {}, io.StringIO(), False
    with contextlib.redirect_stdout(out):
        try:
            K.handle_args(d, BASE + [a.replace("{T}", tmp) for a in argv])
        except SystemExit:
            exited = True
    state = {k: _plain(d[k], tmp) for k in sorted(d) if k.endswith(".spec") or k in ("startFreq", "endFreq", "fullSize")}
    return {"exited": exited, "stdout": out.getvalue().replace(tmp, "<TMP>"), "state": json.loads(json.dumps(state))}


def _kmod():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")


@pytest.fixture(scope="module")
def K():
    return _kmod()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("keys"))
    write_files(tmp)
    return tmp


@pytest.fixture(scope="module")
def recorded():
    with open(TRANSCRIPTS) as f:
        return json.load(f)


def test_the_matrix_is_the_recorded_one(recorded):
    names = [name for name, _ in MATRIX]
    assert len(set(names)) == len(names) and sorted(names) == sorted(recorded)


@pytest.mark.parametrize("name,argv", MATRIX, ids=[name for name, _ in MATRIX])
def test_key_transcript(K, files, recorded, name, argv):
    got, want = transcript(K, argv, files), recorded[name]
    assert got["exited"] == want["exited"], got["stdout"]
    assert got["stdout"] == want["stdout"]
    assert got["state"] == want["state"]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_cli_keys_host.py --record")
    with tempfile.TemporaryDirectory() as tmp:
        write_files(tmp)
        K = _kmod()
        rec = {name: transcript(K, argv, tmp) for name, argv in MATRIX}
    with open(TRANSCRIPTS, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded %d transcripts, %d of them quit" % (len(rec), sum(r["exited"] for r in rec.values())))
