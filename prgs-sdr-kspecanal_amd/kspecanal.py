#!/usr/bin/env python3
"""kSpecAnal front end on the MI355X engine: the reference's zeroSpan / scan command line and plotting
hand-off (python/kspecanal.py, cited "K:") with the numpy.fft hot path replaced by libksa.

    python -m prgs-sdr-kspecanal_amd.kspecanal zeroSpan centerFreq 91.1e6 fftSize 4096 window hanning source synth
    python kspecanal.py fmScan source synth prgLoopCnt 4 bPltLevels false bPltHeatMap false

What is kept from the reference: the case-insensitive `KEY value` grammar and every key (K:813-911), the
mode words and aliases (K:816, K:912-921), the defaults (K:41-59), the dict `d` as the only state carrier
with the same key names, the module-level `sdr_curscan(d)` seam that playback rebinds (K:531, K:543), and the
arrays handed to matplotlib: d['Fft.Cur'|'Fft.Max'|'Fft.Min'|'Fft.Avg'], the freqs axis, and the
[128, W] waterfall buffer (K:470-481, K:729).  New keys are additive: `source` (rtlsdr|synth|file:<path>),
`device`, `iqFormat` (c64|u8|s8|s16), `frameBatch` (zeroSpan blocks per device call, default 1), `pfbTaps` (P >= 1: the
polyphase filter bank front end -- P*fftSize samples per spectrum, weighted by a sinc prototype tapered with `window`, folded
onto fftSize points and transformed once; default 0 = off), `pfbSpectra` (K >= 1, with pfbTaps: the integrating polyphase
spectrometer -- a block of (P+K-1)*fftSize samples holds K such spectra, summed as power, a density; default 0 = off),
`density` (L:lo:hi, zeroSpan only: a density / persistence histogram of every frame's dB spectrum, L levels over [lo, hi) dB
against the waterfall's columns, handed off as d['density'], d['densityNaN'], d['densityEdges'], d['densityRows'];
default empty = off), `densitySave` (a file that takes the [L+1, W] int64 counts, NaN row last, with np.save),
`mask` (flat:U[:L] | file:PATH | learn:F:M, optionally :minBins=K and :events=E, zeroSpan only: a frequency-mask trigger --
every frame's dB spectrum is compared against an upper and a lower limit line, the frames that cross are reported and every
bin counts its crossings; handed off as d['maskEvents'], d['maskEventsTotal'], d['maskHits'], d['maskRows'],
d['maskEventRows']; default empty = off), `maskSave` (an .npz of events, events_total, hits, rows_seen, upper, lower and
event_rows, the dB spectra of the stored events) and `zoom` (D[:offsetHz[:tapsPerPhase]], zeroSpan only: a digital
down-converter in front of the engine -- every frame captures D*(fullSize-1) + D*tapsPerPhase samples, which are mixed down by
offsetHz, low-pass filtered and decimated by D on the GPU, so that the same fftSize spans samplingRate/D around
centerFreq + offsetHz; default empty = off) and `detect` (T:G:THR[:mode=ca|go|so][:minWidth=W][:maxGap=K][:events=E],
zeroSpan only: a CFAR signal detector -- every bin of every frame's dB spectrum is compared against the mean of T training cells
on either side beyond G guard cells plus THR dB, the detected bins are grouped into emissions (start bin, stop bin, peak, floor)
and every bin counts the frames in which it lay inside one; handed off as d['detectEmissions'], d['detectEmissionsTotal'],
d['detectHits'], d['detectRows']; default empty = off), `detectSave` (an .npz of emissions, emissions_total, hits, rows_seen, the
parameters, and every emission's centre and width in Hz), `demod` (MODE[:audioDecim[:tapsPerPhase[:deemphUs]]] with MODE
am|fm|pm, zeroSpan only, needs `zoom` (`zoom 1` passes the whole band): an AM / FM / PM demodulator behind the zoom -- every
frame's zoomed block is turned into amplitude, frequency or phase versus time, low-pass filtered and decimated by audioDecim on
the GPU into int16 PCM; each block is demodulated on its own and the blocks abut in the hand-off and in the file; handed off as
d['demodAudio'] (int16) and d['demodRate']; default empty = off) and `demodSave` (FILE.wav, a mono 16-bit WAV file of that
audio at samplingRate / (zoom D x audioDecim), rounded to an integer), `channels` (M[:O[:tapsPerBranch[:pick]]], zeroSpan only,
instead of `zoom`: a polyphase channelizer in front of the engine -- every frame's capture becomes all M channels of the band at
once, each at samplingRate x O / M, channel `pick` goes on to the engine (and to `demod`, which it satisfies in place of
`zoom`), and the mean power of every channel over the run is handed off as d['channelsPower'] in dB with d['channelsFreqs'];
default empty = off), `channelsSave` (an .npz of power_db, freqs and the parameters) and `audioRate` (HZ[:tapsPerPhase],
zeroSpan only, needs `demod`: the demodulator then leaves float32 audio on the GPU and a polyphase L / M resampler, L / M = HZ
over the demodulator's rate, reduced, turns every block of it into int16 PCM at exactly HZ, which is what d['demodRate'] and the
WAV header then say; default empty = off) and `correlate` (FILE.npy[:threshold[:guard[:events=N]]], zeroSpan only, not with
`zoom` or `channels`: a matched-filter correlator over every frame's raw block -- FILE holds a complex template [K] or a bank
[Q][K]; every lag of every block gets its normalised correlation against each template, and the lags at which it peaks at or
above threshold (default 0.5) within guard lags on either side (default K) are listed; handed off as d['corrEvents'] (block is
the running block index of the run) and d['corrTotal']; default empty = off), `correlateSave` (an .npz of the events, toa =
block, fractional position and seconds inside the block, and the parameters), `pulses`
([rel:]ON_DB:OFF_DB[:W[:minLen[:events=N]]], zeroSpan only, not with `zoom` or `channels`, allowed beside `correlate`: a
time-domain pulse detector over every frame's raw block -- the power summed over W samples (default 16) is compared with a trigger
level that has hysteresis, ON_DB to start a pulse and OFF_DB <= ON_DB to end it, in dB relative to full scale as 10 log10 of the
mean power, or with rel: in dB above the median envelope of the first block; runs shorter than minLen (default 1) are dropped;
handed off as d['pulseEvents'] (block is the running block index of the run), d['pulseTotal'] and d['pulseActive']; default
empty = off), `pulsesSave` (an .npz of the records, both totals, the parameters, and every pulse's toa_s, width_s, mean_dbfs,
peak_dbfs and freq_hz), `track` (GAP:SLOP[:minRows=R][:minSpans=S][:events=E], zeroSpan only, needs `detect`: at the end of the
run the detector's emissions are linked on the GPU into time-frequency tracks -- emissions at most GAP missing frames apart whose
bins overlap or miss each other by at most SLOP bins are one track, tracks over fewer than R frames or of fewer than S emissions
are dropped; handed off as d['trackTracks'], d['trackTotal'], d['trackComponents'] and d['trackLabels'], the track of every
stored emission; default empty = off) and `trackSave` (an .npz of the records, both totals, the labels, the parameters, and
every track's t_start_s, duration_s, center_hz, width_hz and drift_hz_per_s), `iqfix` (MODE[:blocks=N][:track] with MODE
dc|iq|dc+iq, zeroSpan only, not with `channels`, `correlate`, `pulses` or bUsePSD true: a blind DC-offset and IQ-imbalance
corrector in front of everything else -- the sums of the first N blocks of the first batch (default all of it) are solved into a
correction that every block of the run then gets before the engine (or `zoom`) sees it; with track every batch is corrected
with the coefficients solved from the batch before it; handed off as d['iqfix'], a dict of per-solve arrays; default empty =
off) and `iqfixSave` (an .npz of those arrays: batch, dc_i, dc_q, c, d, flags, count, sums, gain_db and phase_deg per solve),
`continuous` (true|false, zeroSpan only, not with bUsePSD true: the raw blocks of the run are read back to back -- no sample of
the source is dropped between them (sources.ContiguousReader) -- and taken as ONE stream, and the stages that have a stream form
run it with their state carried on the GPU from batch to batch: `zoom` and `channels` then capture exactly D x fullSize samples
per frame, the mixer phase and the filter history run on, and channels keeps its start-up transient; `demod` and `audioRate`
give seamless audio of ceil(frames x fullSize / audioDecim) samples (times L / M, rounded up) with no seam at a block edge;
`pulses` and `correlate` find what straddles a block edge once, their records carry block -1 and positions counted from the
run's first sample, and the hand-off flushes them, so that a pulse still on at the end is listed with its open-end flag; the
engine takes every batch one frame per call, so that Fft.Avg is the per-frame recursion and nothing handed off depends on
frameBatch; default false = every block is a capture of its own, the reference's model), `measure` (B[:xdb=X][:margin=M] with the
occupied percentage 50 <= B < 100, zeroSpan only, needs `detect`: a band meter beside the detector -- after every batch the new
emissions are measured on the GPU in the rows they were found in, each over its span widened by M bins (default 0) on either
side: integrated power, power centroid, peak, the occupied bandwidth that holds B % of the power and the width X dB (default 3)
below the peak; result i belongs to emission i; handed off as d['measureResults']; default empty = off) and `measureSave` (an
.npz of the records, the parameters, and per record center_hz -- the power centroid --, obw_hz, xdb_hz, power_net_db -- the power
less the detector's floor over the window -- and snr_db, that net power over the floor's).
The scan modes have keys of their own: `scanDetect` (T:G:THR[:mode=ca|go|so][:minWidth=W][:maxGap=K][:events=E][:edge=K][:dc=K],
scan modes only: the CFAR detector of `detect` over every tuned band's dB row of every pass -- each band has its own gain and
floor --, the band emissions mapped to the stitched range and the sightings that overlapping bands give of one emission joined
into one record per pass (survey.stitch_emissions); dc=K drops what lies within K bins of a band's centre, the receiver's
spike, edge=K what peaks in the outer K bins of a band while another band sees the same frequency further inside; events is
the room of the run's list, whose total counts every emission; handed off as d['surveyEmissions'] (row is the pass, the bins
index d['freqsAll']), d['surveyMembers'], d['surveyEmissionsTotal'], d['surveyCounters'], d['surveyOccupancy'] (per xRes cell,
the passes in which an emission touched it) and d['surveyPasses']; default empty = off), `scanDetectSave` (an .npz of those, the
parameters, and every emission's centre, width and peak in Hz), `scanTrack` (GAP:SLOP[:minRows=R][:minSpans=S][:events=E], scan
modes only, needs `scanDetect`: at the end of the run the stored emissions are linked on the GPU over the passes -- GAP in
missing passes, SLOP in stitched bins; handed off as d['surveyTracks'], d['surveyTrackTotal'], d['surveyTrackComponents'] and
d['surveyTrackLabels']; default empty = off) and `scanTrackSave` (an .npz like trackSave's, a row being a pass of the measured
mean duration).
What moved to the GPU:
everything from the IQ block to those arrays.
Deliberate differences: playback needs no SDR; in scan mode the Levels plot is
refreshed once per pass (the whole pass is one device call) instead of once per tuned band, and in zeroSpan with
frameBatch > 1 once per batch.
Hand-off traffic: with a decimating pltCompress (AVG|MAX|MIN) a frame / pass brings back the four
xRes-point Levels curves, the peak markers and the ONE new waterfall row (ksa_read_view, d['handoff.bytes']); the
full-width d['Fft.*'] arrays are read from the device when a RAW / CONV plot needs them and once at the end of a run:
DURING such a run they are None / stale (the reference refreshes them after every frame, K:470-476) -- code that reads
d['Fft.*'] between frames calls _materialize(d, d['ksa.engine'], scan) first.
"""
import collections
import pickle
import signal
import sys
import time

import numpy as np

from . import engine as _engine
from .engine import SpectrumEngine, KsaError, FMT_C64, FMT_U8, FMT_S8, FMT_S16
from . import sources
from .density import SpectrumDensity
from .mask import SpectrumMask, learn_mask, EVENT_DTYPE, MAX_CAPACITY
from .ddc import DownConverter, ddc_lowpass, MAX_DECIM, MAX_TAPS, MAX_IN
from . import detect as _detect
from .detect import SignalDetector, emission_freqs
from . import demod as _demod
from .demod import Demodulator, demod_taps, write_wav
from . import chan as _chan
from .chan import Channelizer, chan_prototype, channel_freqs
from . import resamp as _resamp
from .resamp import Resampler, resample_taps, rate_ratio
from . import corr as _corr
from .corr import Correlator, refine
from . import pulse as _pulse
from .pulse import PulseDetector
from . import track as _track
from .track import EmissionTracker, track_times_freqs
from . import iqfix as _iqfix
from .iqfix import IqCorrector
from .survey import ScanSurvey
from . import measure as _measure
from .measure import SpectrumMeter, result_freqs

IQFORMATS = ("c64", "u8", "s8", "s16")      # s8 / s16: interleaved signed int8 (b / 128) / little-endian int16 (b / 32768) I,Q
PRGMODES = ("ZEROSPAN", "ZEROSPANSAVE", "ZEROSPANPLAY", "SCAN", "FMSCAN", "QUICKFULLSCAN")
PLTCOMPRESS = ("MAX", "MIN", "AVG", "RAW", "CONV")

# key -> (dict name, parser); the reference's spelling is matched case-insensitively (K:815)
def _arg_boolean(v):
    """K:771-775."""
    return v.upper() == "TRUE"


_bool = _arg_boolean
_KEYS = {
    "CENTERFREQ": ("centerFreq", float), "STARTFREQ": ("startFreq", float), "ENDFREQ": ("endFreq", float),
    "SAMPLINGRATE": ("samplingRate", float), "GAIN": ("gain", float), "MINAMP4CLIP": ("minAmp4Clip", float),
    "CURSCANNONOVERLAP": ("curScanNonOverlap", float), "CURSCANCUMUMODE": ("curScanCumuMode", str.upper),
    "SCANRANGENONOVERLAP": ("scanRangeNonOverlap", float), "FFTSIZE": ("fftSize", int), "XRES": ("xRes", int),
    "BDATAMIN": ("bDataMin", _bool), "BDATAMAX": ("bDataMax", _bool), "BDATAAVG": ("bDataAvg", _bool),
    "BDATACUR": ("bDataCur", _bool), "PLTCOMPRESS": ("pltCompress", str.upper),
    "WINDOW": ("window", lambda v: "WIN." + v.upper()), "BPLTHEATMAP": ("bPltHeatMap", _bool),
    "BPLTLEVELS": ("bPltLevels", _bool), "PRGLOOPCNT": ("prgLoopCnt", int),
    "PLTHIGHSNUMMARKERS": ("pltHighsNumMarkers", int), "PLTHIGHSDELTA4MARKING": ("pltHighsDelta4Marking", float),
    "PLTHIGHSPAUSE": ("pltHighsPause", _bool), "SAVESIGLVLS": ("SaveSigLvls", str), "ADJSIGLVLS": ("AdjSigLvls", str),
    "BGRID": ("bGrid", _bool), "BUSEPSD": ("bUsePSD", _bool),
    "BSCANRANGEBASEDATAISRAW": ("bScanRangeBaseDataIsRaw", _bool),
    "ZEROSPANSAVEFILE": ("zeroSpanSaveFile", str), "ZEROSPANPLAYFILE": ("zeroSpanPlayFile", str),
    # additive keys of this build
    "SOURCE": ("source", str), "DEVICE": ("device", int), "IQFORMAT": ("iqFormat", str.lower),
    "FRAMEBATCH": ("frameBatch", int), "PFBTAPS": ("pfbTaps", int), "PFBSPECTRA": ("pfbSpectra", int),
    "DENSITY": ("density", str), "DENSITYSAVE": ("densitySave", str), "MASK": ("mask", str), "MASKSAVE": ("maskSave", str),
    "ZOOM": ("zoom", str), "DETECT": ("detect", str), "DETECTSAVE": ("detectSave", str),
    "DEMOD": ("demod", str), "DEMODSAVE": ("demodSave", str),
    "CHANNELS": ("channels", str), "CHANNELSSAVE": ("channelsSave", str), "AUDIORATE": ("audioRate", str),
    "CORRELATE": ("correlate", str), "CORRELATESAVE": ("correlateSave", str),
    "PULSES": ("pulses", str), "PULSESSAVE": ("pulsesSave", str),
    "TRACK": ("track", str), "TRACKSAVE": ("trackSave", str),
    "IQFIX": ("iqfix", str.lower), "IQFIXSAVE": ("iqfixSave", str),
    "SCANDETECT": ("scanDetect", str), "SCANDETECTSAVE": ("scanDetectSave", str),
    "SCANTRACK": ("scanTrack", str), "SCANTRACKSAVE": ("scanTrackSave", str),
    "CONTINUOUS": ("continuous", _bool),
}
# the keys of the band meter, beside _KEYS: same grammar, looked up after it
_KEYS_MEASURE = {"MEASURE": ("measure", str), "MEASURESAVE": ("measureSave", str)}


def defaults():
    """K:41-74 and K:783-812."""
    return {
        "prgMode": "FMSCAN", "samplingRate": 2.4e6, "gain": 19.1, "centerFreq": 92e6, "fftSize": 2 ** 14,
        "curScanNonOverlap": 0.1, "curScanCumuMode": "AVG", "window": "WIN.ONES",
        "minAmp4Clip": (1 / 256) * 0.00001, "bPltHeatMap": True, "bPltLevels": True,
        "scanRangeNonOverlap": 0.5, "prgLoopCnt": 8192, "xRes": 512, "pltCompress": "AVG",
        "pltHighsNumMarkers": 5, "pltHighsDelta4Marking": 0.025, "pltHighsPause": False, "pltCompressHM": "MAX",
        "SaveSigLvls": "", "AdjSigLvls": "", "bDataMin": True, "bDataMax": True, "bDataAvg": True, "bDataCur": True,
        "bGrid": True, "bUsePSD": False, "bScanRangeBaseDataIsRaw": False,
        "zeroSpanSaveFile": "/tmp/zerospan.save", "zeroSpanPlayFile": "/tmp/zerospan.save",
        "source": "rtlsdr", "device": 0, "iqFormat": "c64", "frameBatch": 1, "pfbTaps": 0, "pfbSpectra": 0, "cmd.stop": False,
        "density": "", "densitySave": "", "mask": "", "maskSave": "", "zoom": "",
        "detect": "", "detectSave": "", "demod": "", "demodSave": "", "channels": "", "channelsSave": "",
        "audioRate": "", "correlate": "", "correlateSave": "", "pulses": "", "pulsesSave": "",
        "track": "", "trackSave": "", "iqfix": "", "iqfixSave": "",
        "scanDetect": "", "scanDetectSave": "", "scanTrack": "", "scanTrackSave": "", "continuous": False,
        "measure": "", "measureSave": "",
    }


def prg_quit(d, msg=None, tryExit=True):
    """K:967-972."""
    if msg is not None:
        print(msg)
    d["cmd.stop"] = True
    if tryExit:
        sys.exit()


def _fixupfreqs_scanrange(d):
    """K:701-709: stretch endFreq so that the range is a whole number of sampling-rate bands."""
    bands = (d["endFreq"] - d["startFreq"]) / d["samplingRate"]
    if (bands % 1) != 0:
        d["orig.EndFreq"] = d["endFreq"]
        d["endFreq"] = d["startFreq"] + np.ceil(bands) * d["samplingRate"]
        print("WARN:scanRange:Adjusting endFreq: orig [{}] adjusted [{}], so that fullRange is Multiple of samplingRate/freqBand [{}]".format(
            d["orig.EndFreq"], d["endFreq"], d["samplingRate"]))
    d["centerFreq"] = d["startFreq"] + ((d["endFreq"] - d["startFreq"]) / 2)


def handle_args(d, argv=None):
    """Fill `d` with the defaults and the user's KEY value pairs (K:778-949)."""
    for k, v in defaults().items():
        if not (k == "cmd.stop" and k in d):
            d[k] = v
    argv = list(sys.argv[1:] if argv is None else argv)
    i = 0
    while i < len(argv):
        cur = argv[i].upper()
        if cur in PRGMODES:
            d["prgMode"] = cur
        elif cur in _KEYS or cur in _KEYS_MEASURE:
            if i + 1 >= len(argv):
                prg_quit(d, "ERROR:handle_args: Missing value for [{}]".format(cur))
            name, parse = _KEYS[cur] if cur in _KEYS else _KEYS_MEASURE[cur]
            i += 1
            d[name] = parse(argv[i])
        else:
            prg_quit(d, "ERROR:handle_args: Unknown argument [{}]".format(cur))
        i += 1
    if d["prgMode"] == "FMSCAN":                                   # K:912-915
        d["prgMode"], d["startFreq"], d["endFreq"] = "SCAN", 88e6, 108e6
    elif d["prgMode"] == "QUICKFULLSCAN":                          # K:916-921
        d["prgMode"], d["startFreq"], d["endFreq"] = "SCAN", 30e6, 1.5e9
        d["fftSize"], d["pltCompress"] = 64, "RAW"
    if d["prgMode"] == "SCAN":
        _fixupfreqs_scanrange(d)
    else:
        d["startFreq"] = d["centerFreq"] - d["samplingRate"] / 2   # K:275-278
        d["endFreq"] = d["centerFreq"] + d["samplingRate"] / 2
    d["fullSize"] = _engine.full_size_for(d["fftSize"], d["samplingRate"])
    for name in ("HAMMING", "HANNING", "KAISER", "ONES"):         # K:932-935
        d["WIN." + name] = _engine.window_table(name, d["fftSize"])
    if d["window"] not in d:
        prg_quit(d, "ERROR:handle_args: Unknown window [{}]".format(d["window"]))
    d["theWin"] = d[d["window"]]
    if d["xRes"] > d["fftSize"]:                                   # K:938-940
        print("WARN:fftSize[{}] < xRes[{}], setting xRes to fftSize".format(d["fftSize"], d["xRes"]))
        d["xRes"] = d["fftSize"]
    elif d["fftSize"] % d["xRes"] != 0:                            # K:941-949
        for div in range(int(d["fftSize"] / 300), 0, -1):
            if d["fftSize"] % div == 0:
                new = d["fftSize"] // div
                print("WARN:fftSize[{}] NotMultipleOf xRes[{}], setting xRes to {}".format(d["fftSize"], d["xRes"], new))
                d["xRes"] = new
                break
    if not _engine.fft_size_supported(d["fftSize"]):             # the engine's sizes (the reference takes any, K:391)
        prg_quit(d, "ERROR:handle_args: " + _engine.fft_size_message(d["fftSize"]))
    if d["curScanCumuMode"] not in ("AVG", "MAX", "MIN", "RAW", "PSD"):   # PSD: the Welch fold on the device (additive)
        prg_quit(d, "ERROR: Unknown cumuMode [{}], Quiting...".format(d["curScanCumuMode"]))
    if d["iqFormat"] not in IQFORMATS:
        prg_quit(d, "ERROR:handle_args: Unknown iqFormat [{}], expected one of {}".format(d["iqFormat"], "|".join(IQFORMATS)))
    if d["frameBatch"] < 1:
        prg_quit(d, "ERROR:handle_args: frameBatch [{}] must be >= 1".format(d["frameBatch"]))
    if d["bUsePSD"] and d["frameBatch"] > 1:
        prg_quit(d, "ERROR:handle_args: frameBatch [{}] needs bUsePSD false: the PSD diagnostic is per block".format(d["frameBatch"]))
    for handle in _HANDLERS:
        handle(d)
    return d


# ---------------------------------------------------------------------- what the handlers of the additive zeroSpan keys share
def _key_text(d, key, spec_key, save=None):
    """Opens a handler: d[spec_key] = None, and the key's text -- or, when the key is off, None after the warning about a save
    key that was given without it."""
    d[spec_key] = None
    if not d[key] and save and d[save]:
        print("WARN:handle_args: {} [{}] is ignored without {}".format(save, d[save], key))
    return d[key] or None


def _refuse(d, key, text, rule):
    prg_quit(d, "ERROR:handle_args: {} [{}]: {}".format(key, text, rule))


def _gate(d, key, text, psd_reason=None):
    """Where a zeroSpan-only key may run: True (after the warning) when playback ignores it, a quit in any other mode, and a
    quit under bUsePSD when the key gives a reason why it cannot run beside the PSD diagnostic."""
    if d["prgMode"] == "ZEROSPANPLAY":
        print("WARN:handle_args: {} [{}] is ignored when playing saved spectra".format(key, text))
        return True
    if d["prgMode"] != "ZEROSPAN":
        prg_quit(d, "ERROR:handle_args: {} [{}] is zeroSpan only, prgMode is [{}]".format(key, text, d["prgMode"]))
    if psd_reason and d["bUsePSD"]:
        prg_quit(d, "ERROR:handle_args: {} [{}] needs bUsePSD false: {}".format(key, text, psd_reason))
    return False


def _options(parts, spec, names):
    """The optional name=value suffixes of a key, in any order, each at most once: `names` maps the lower-cased names to the
    fields of `spec`, whose defaults tell a word from an integer.  ValueError on an unknown name, a missing = or a repeat."""
    seen = set()
    for part in parts:
        name, eq, value = part.partition("=")
        key = names.get(name.lower())
        if not eq or key is None or key in seen:
            raise ValueError(part)
        seen.add(key)
        spec[key] = value.lower() if isinstance(spec[key], str) else int(value)


DENSITY_RULE = "density wants L:lo:hi with an integer 1 <= L <= 1024 levels and finite lo < hi in dB"


def _handle_density(d):
    """density L:lo:hi (additive, zeroSpan only): d['density.spec'] = (L, lo, hi), or None when the key is off."""
    text = _key_text(d, "density", "density.spec", "densitySave")
    if not text:
        return
    try:
        levels, lo, hi = text.split(":")
        levels, lo, hi = int(levels), float(lo), float(hi)
    except ValueError:
        _refuse(d, "density", text, DENSITY_RULE)
    if not (1 <= levels <= 1024 and np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        _refuse(d, "density", text, DENSITY_RULE)
    if _gate(d, "density", text, "it counts the engine's own dB rows"):
        return
    d["density.spec"] = (levels, lo, hi)


MASK_RULE = ("mask wants flat:U[:L] (dB, L <= U), file:PATH (an .npy of [fftSize] or [2][fftSize] values, upper then lower, no NaN, "
             "lower <= upper) or learn:F:M (the first F >= 1 frames plus M dB), optionally followed by :minBins=K (1..fftSize) "
             "and :events=E (1..%d)" % MAX_CAPACITY)


def _handle_mask(d):
    """mask flat:U[:L] | file:PATH | learn:F:M, with optional :minBins=K and :events=E (additive, zeroSpan only):
    d['mask.spec'] = dict(kind, upper, lower, frames, margin, min_bins, capacity), or None when the key is off."""
    text = _key_text(d, "mask", "mask.spec", "maskSave")
    if not text:
        return

    def refuse():
        _refuse(d, "mask", text, MASK_RULE)

    n = d["fftSize"]
    spec = dict(kind=None, upper=None, lower=None, frames=0, margin=0.0, min_bins=1, capacity=4096)
    names = {"minbins": "min_bins", "events": "capacity"}
    body, opts = text, []
    try:
        while True:                                  # peeled from the right: the PATH of file: may hold colons
            head, sep, last = body.rpartition(":")
            name, eq, _ = last.partition("=")
            if not sep or not eq or name.lower() not in names:
                break
            body = head
            opts.append(last)
        _options(opts, spec, names)
        kind, _, rest = body.partition(":")
        spec["kind"] = kind = kind.lower()
        if kind == "flat":
            vals = [float(v) for v in rest.split(":")]
            if len(vals) not in (1, 2) or any(np.isnan(v) for v in vals) or (len(vals) == 2 and vals[1] > vals[0]):
                raise ValueError(text)
            spec["upper"] = np.full(n, vals[0], dtype=np.float32)
            spec["lower"] = np.full(n, vals[1], dtype=np.float32) if len(vals) == 2 else None
        elif kind == "file":
            if not rest:
                raise ValueError(text)
            spec["path"] = rest
        elif kind == "learn":
            frames, margin = rest.split(":")
            spec["frames"], spec["margin"] = int(frames), float(margin)
            if spec["frames"] < 1 or not np.isfinite(spec["margin"]):
                raise ValueError(text)
        else:
            raise ValueError(text)
        if not (1 <= spec["min_bins"] <= n and 1 <= spec["capacity"] <= MAX_CAPACITY):
            raise ValueError(text)
    except ValueError:
        refuse()
    if _gate(d, "mask", text, "it checks the engine's own dB rows"):
        return
    if kind == "file":
        try:
            a = np.asarray(np.load(spec["path"], allow_pickle=False), dtype=np.float32)
        except (OSError, ValueError, TypeError):
            refuse()
        if a.shape == (n,):
            spec["upper"] = a
        elif a.shape == (2, n):
            spec["upper"], spec["lower"] = np.ascontiguousarray(a[0]), np.ascontiguousarray(a[1])
        else:
            refuse()
        if np.isnan(a).any() or (spec["lower"] is not None and np.any(spec["lower"] > spec["upper"])):
            refuse()
    d["mask.spec"] = spec


def _handle_continuous(d):
    """continuous true|false (additive, zeroSpan only): the raw blocks of the run are one back-to-back stream and every stage
    that has a stream form runs it.  It stands in front of the handlers whose specs it changes (zoom, channels, demod,
    audioRate); false, the default, changes nothing."""
    if not d["continuous"]:
        return
    if _gate(d, "continuous", "true", "the PSD diagnostic is per block"):
        d["continuous"] = False


ZOOM_RULE = ("zoom wants D[:offsetHz[:tapsPerPhase]] with an integer 1 <= D <= %d, a finite |offsetHz| <= samplingRate/2 and an "
             "integer 1 <= tapsPerPhase <= 16 with D x tapsPerPhase <= %d (defaults: offsetHz 0, tapsPerPhase 8); a batch of "
             "D x (fullSize - 1) + D x tapsPerPhase samples per frame must stay below 2^28 samples" % (MAX_DECIM, MAX_TAPS))


def _handle_zoom(d):
    """zoom D[:offsetHz[:tapsPerPhase]] (additive, zeroSpan only): the digital down-converter in front of the engine.
    d['zoom.spec'] = dict(decim, offset, taps_per_phase, ntaps, block_len, center, span), or None when the key is off; startFreq
    and endFreq become those of the zoomed span."""
    text = _key_text(d, "zoom", "zoom.spec")
    if not text:
        return
    try:
        parts = text.split(":")
        if not 1 <= len(parts) <= 3:
            raise ValueError(text)
        decim = int(parts[0])
        offset = float(parts[1]) if len(parts) > 1 else 0.0
        tpp = int(parts[2]) if len(parts) > 2 else 8
        if not (1 <= decim <= MAX_DECIM and np.isfinite(offset) and abs(offset) <= d["samplingRate"] / 2
                and 1 <= tpp <= 16 and decim * tpp <= MAX_TAPS):
            raise ValueError(text)
    except ValueError:
        _refuse(d, "zoom", text, ZOOM_RULE)
    if _gate(d, "zoom", text, "the PSD diagnostic sees the whole band"):
        return
    ntaps = decim * tpp
    # continuous: the filter's history is carried from block to block, so a frame costs exactly decim x fullSize samples
    block_len = decim * d["fullSize"] if d["continuous"] else decim * (d["fullSize"] - 1) + ntaps
    if d["frameBatch"] * block_len > MAX_IN:
        _refuse(d, "zoom", text, ZOOM_RULE)
    center, span = d["centerFreq"] + offset, d["samplingRate"] / decim
    d["zoom.spec"] = dict(decim=decim, offset=offset, taps_per_phase=tpp, ntaps=ntaps, block_len=block_len, center=center, span=span)
    d["startFreq"], d["endFreq"] = center - span / 2, center + span / 2


CHANNELS_RULE = ("channels wants M[:O[:tapsPerBranch[:pick]]] with M a power of two %d <= M <= %d, O 1, 2 or 4 with O <= M, an "
                 "integer 1 <= tapsPerBranch <= %d with M x tapsPerBranch <= %d and a channel 0 <= pick < M (defaults: O 2, "
                 "tapsPerBranch 8, pick 0); a batch of (M / O) x (ceil((M x tapsPerBranch - 1) / (M / O)) + fullSize - 1) + 1 samples "
                 "per frame must stay below 2^28 samples" % (_chan.MIN_CHAN, _chan.MAX_CHAN, _chan.MAX_BRANCH_TAPS, _chan.MAX_TAPS))


def _handle_channels(d):
    """channels M[:O[:tapsPerBranch[:pick]]] (additive, zeroSpan only, instead of zoom): the polyphase channelizer in front of
    the engine.  d['chan.spec'] = dict(nchan, oversample, taps_per_branch, pick, decim, ntaps, first, block_len, offset, center,
    span), or None when the key is off; startFreq and endFreq become those of the picked channel."""
    text = _key_text(d, "channels", "chan.spec", "channelsSave")
    if not text:
        return
    try:
        parts = text.split(":")
        if not 1 <= len(parts) <= 4:
            raise ValueError(text)
        nchan = int(parts[0])
        over = int(parts[1]) if len(parts) > 1 else 2
        tpb = int(parts[2]) if len(parts) > 2 else 8
        pick = int(parts[3]) if len(parts) > 3 else 0
        if not (_chan.MIN_CHAN <= nchan <= _chan.MAX_CHAN and nchan & (nchan - 1) == 0 and over in (1, 2, 4) and over <= nchan
                and 1 <= tpb <= _chan.MAX_BRANCH_TAPS and nchan * tpb <= _chan.MAX_TAPS and 0 <= pick < nchan):
            raise ValueError(text)
    except ValueError:
        _refuse(d, "channels", text, CHANNELS_RULE)
    if _gate(d, "channels", text, "the PSD diagnostic sees the whole band"):
        return
    if d["zoom.spec"] is not None:
        prg_quit(d, "ERROR:handle_args: channels [{}] and zoom [{}] exclude each other: either is the front end of the engine".format(
            text, d["zoom"]))
    decim, ntaps = nchan // over, nchan * tpb
    if d["continuous"]:                      # the stream form: no column is dropped, the start-up transient is part of the stream
        first, block_len = 0, decim * d["fullSize"]
    else:
        first = -(-(ntaps - 1) // decim)
        block_len = decim * (first + d["fullSize"] - 1) + 1
    if d["frameBatch"] * block_len > _chan.MAX_IN:
        _refuse(d, "channels", text, CHANNELS_RULE)
    offset = float(channel_freqs(nchan, d["samplingRate"])[pick])
    center, span = d["centerFreq"] + offset, d["samplingRate"] / decim
    d["chan.spec"] = dict(nchan=nchan, oversample=over, taps_per_branch=tpb, pick=pick, decim=decim, ntaps=ntaps, first=first,
                          block_len=block_len, offset=offset, center=center, span=span)
    d["startFreq"], d["endFreq"] = center - span / 2, center + span / 2


DETECT_RULE = ("detect wants T:G:THR with integers 1 <= T <= %d training and 0 <= G <= %d guard cells on either side and a finite "
               "threshold 0 <= THR <= 100 in dB, optionally followed by :mode=ca|go|so, :minWidth=W (1..fftSize), :maxGap=K (0..%d) "
               "and :events=E (1..%d), each at most once; fftSize %d..%d" % (
                   _detect.MAX_TRAIN, _detect.MAX_GUARD, _detect.MAX_GAP, _detect.MAX_CAPACITY, _detect.MIN_NBINS, _detect.MAX_NBINS))


def _handle_detect(d):
    """detect T:G:THR[:mode=ca|go|so][:minWidth=W][:maxGap=K][:events=E] (additive, zeroSpan only): d['detect.spec'] =
    dict(train, guard, threshold, mode, min_width, max_gap, capacity), or None when the key is off."""
    text = _key_text(d, "detect", "detect.spec", "detectSave")
    if not text:
        return
    n = d["fftSize"]
    spec = dict(train=0, guard=0, threshold=0.0, mode="ca", min_width=1, max_gap=0, capacity=4096)
    try:
        parts = text.split(":")
        if len(parts) < 3:
            raise ValueError(text)
        spec["train"], spec["guard"], spec["threshold"] = int(parts[0]), int(parts[1]), float(parts[2])
        _options(parts[3:], spec, {"mode": "mode", "minwidth": "min_width", "maxgap": "max_gap", "events": "capacity"})
        if not (1 <= spec["train"] <= _detect.MAX_TRAIN and 0 <= spec["guard"] <= _detect.MAX_GUARD
                and np.isfinite(spec["threshold"]) and 0 <= spec["threshold"] <= 100 and spec["mode"] in _detect.MODES
                and 1 <= spec["min_width"] <= n and 0 <= spec["max_gap"] <= _detect.MAX_GAP
                and 1 <= spec["capacity"] <= _detect.MAX_CAPACITY and _detect.MIN_NBINS <= n <= _detect.MAX_NBINS):
            raise ValueError(text)
    except ValueError:
        _refuse(d, "detect", text, DETECT_RULE)
    if _gate(d, "detect", text, "it reads the engine's own dB rows"):
        return
    d["detect.spec"] = spec


TRACK_RULE = ("track wants GAP:SLOP with integers 0 <= GAP <= %d missing frames and 0 <= SLOP <= fftSize bins, optionally followed "
              "by :minRows=R (>= 1), :minSpans=S (>= 1) and :events=E (1..%d, default 4096), each at most once" % (
                  _track.MAX_ROW_GAP, _track.MAX_CAPACITY))


def _handle_track(d):
    """track GAP:SLOP[:minRows=R][:minSpans=S][:events=E] (additive, zeroSpan only, needs detect): d['track.spec'] =
    dict(row_gap, bin_slop, min_rows, min_spans, capacity), or None when the key is off."""
    text = _key_text(d, "track", "track.spec", "trackSave")
    if not text:
        return
    spec = dict(row_gap=0, bin_slop=0, min_rows=1, min_spans=1, capacity=4096)
    try:
        parts = text.split(":")
        if len(parts) < 2:
            raise ValueError(text)
        spec["row_gap"], spec["bin_slop"] = int(parts[0]), int(parts[1])
        _options(parts[2:], spec, {"minrows": "min_rows", "minspans": "min_spans", "events": "capacity"})
        if not (0 <= spec["row_gap"] <= _track.MAX_ROW_GAP and 0 <= spec["bin_slop"] <= d["fftSize"]
                and 1 <= spec["min_rows"] < 2 ** 31 and 1 <= spec["min_spans"] < 2 ** 31
                and 1 <= spec["capacity"] <= _track.MAX_CAPACITY):
            raise ValueError(text)
    except ValueError:
        _refuse(d, "track", text, TRACK_RULE)
    if _gate(d, "track", text):
        return
    if d["detect.spec"] is None:
        prg_quit(d, "ERROR:handle_args: track [{}] links the emissions of detect: give [detect T:G:THR] as well".format(text))
    d["track.spec"] = spec


MEASURE_RULE = ("measure wants B with the occupied percentage 50 <= B < 100, optionally followed by :xdb=X (finite, 0..100 dB below "
                "the peak, default 3) and :margin=M (an integer 0..%d bins on either side of the span, default 0), each at most "
                "once" % _measure.MAX_MARGIN)


def _handle_measure(d):
    """measure B[:xdb=X][:margin=M] (additive, zeroSpan only, needs detect): d['measure.plan'] = dict(percent, occupied, xdb,
    margin); when the key is off there is no such entry."""
    d.pop("measure.plan", None)
    text = d["measure"] or None
    if not text:
        if d["measureSave"]:
            print("WARN:handle_args: measureSave [{}] is ignored without measure".format(d["measureSave"]))
        return
    plan = dict(percent=0.0, occupied=0.0, xdb=3.0, margin=0)
    try:
        parts = text.split(":")
        plan["percent"] = float(parts[0])
        seen = set()
        for part in parts[1:]:
            name, eq, value = part.partition("=")
            name = name.lower()
            if not eq or name not in ("xdb", "margin") or name in seen:
                raise ValueError(part)
            seen.add(name)
            plan[name] = float(value) if name == "xdb" else int(value)
        plan["occupied"] = float(np.float32(plan["percent"] / 100))      # the float32 the meter gets
        if not (50 <= plan["percent"] < 100 and 0.5 <= plan["occupied"] < 1 and np.isfinite(plan["xdb"])
                and 0 <= plan["xdb"] <= 100 and 0 <= plan["margin"] <= _measure.MAX_MARGIN):
            raise ValueError(text)
    except ValueError:
        _refuse(d, "measure", text, MEASURE_RULE)
    if _gate(d, "measure", text, "it reads the engine's own dB rows"):
        return
    if d["detect.spec"] is None:
        prg_quit(d, "ERROR:handle_args: measure [{}] measures the emissions of detect: give [detect T:G:THR] as well".format(text))
    d["measure.plan"] = plan


CORR_RULE = ("correlate wants FILE.npy[:threshold[:guard[:events=N]]] with a finite 0 < threshold <= 1 (default 0.5), an integer "
             "1 <= guard <= %d lags (default K, the template length) and 1 <= N <= %d events (default 4096)" % (
                 _corr.MAX_GUARD, _corr.MAX_CAPACITY))
CORR_FILE_RULE = ("a complex template [K] or bank [Q][K] with 1 <= K <= %d, 1 <= Q <= %d, Q x K <= %d, every value finite and no "
                  "template all zero" % (_corr.MAX_K, _corr.MAX_Q, _corr.MAX_TEMPLATE_VALUES))


def _handle_correlate(d):
    """correlate FILE.npy[:threshold[:guard[:events=N]]] (additive, zeroSpan only): d['corr.spec'] = dict(file, templates,
    threshold, guard, capacity), or None when the key is off."""
    text = _key_text(d, "correlate", "corr.spec", "correlateSave")
    if not text:
        return
    spec = dict(file="", templates=None, threshold=0.5, guard=None, capacity=4096)
    try:
        parts = text.split(":")
        if len(parts) > 4 or not parts[0]:
            raise ValueError(text)
        spec["file"] = parts[0]
        if len(parts) > 1:
            spec["threshold"] = float(parts[1])
        if len(parts) > 2:
            spec["guard"] = int(parts[2])
        _options(parts[3:], spec, {"events": "capacity"})
        if not (np.isfinite(spec["threshold"]) and 0 < spec["threshold"] <= 1 and 1 <= spec["capacity"] <= _corr.MAX_CAPACITY
                and (spec["guard"] is None or 1 <= spec["guard"] <= _corr.MAX_GUARD)):
            raise ValueError(text)
    except ValueError:
        _refuse(d, "correlate", text, CORR_RULE)
    try:
        t = np.load(spec["file"], allow_pickle=False)
        if not (isinstance(t, np.ndarray) and np.iscomplexobj(t) and t.ndim in (1, 2)):
            raise ValueError(text)
        t = np.ascontiguousarray(t.reshape(1, -1) if t.ndim == 1 else t, dtype=np.complex64)
        q, k = t.shape
        if not (1 <= k <= _corr.MAX_K and 1 <= q <= _corr.MAX_Q and q * k <= _corr.MAX_TEMPLATE_VALUES
                and np.all(np.isfinite(t.view(np.float32))) and np.all(np.abs(t).max(axis=1) > 0)):
            raise ValueError(text)
    except (OSError, ValueError):
        prg_quit(d, "ERROR:handle_args: correlate [{}]: the file [{}] must hold {}".format(text, spec["file"], CORR_FILE_RULE))
    spec["templates"] = t
    if spec["guard"] is None:
        spec["guard"] = k
    if _gate(d, "correlate", text):
        return
    if d["zoom"] or d["channels"]:
        prg_quit(d, "ERROR:handle_args: correlate [{}] reads the raw blocks: correlating behind zoom or channels is out of scope, "
                    "drop [{}]".format(text, "zoom" if d["zoom"] else "channels"))
    if d["fullSize"] < k:
        prg_quit(d, "ERROR:handle_args: correlate [{}]: a block of fullSize [{}] samples is shorter than the template of [{}]".format(
            text, d["fullSize"], k))
    d["corr.spec"] = spec


PULSE_RULE = ("pulses wants [rel:]ON_DB:OFF_DB[:W[:minLen[:events=N]]] with finite levels OFF_DB <= ON_DB in dB relative to full "
              "scale (10 log10 of the mean power, at most %.2f; with rel: in dB above the median envelope of the first block), an "
              "integer 1 <= W <= %d samples (default 16), 1 <= minLen <= %d samples (default 1) and 1 <= N <= %d events (default "
              "1024)" % (10 * np.log10(4.0), _pulse.MAX_W, _pulse.MAX_MIN_LEN, _pulse.MAX_CAPACITY))


def _handle_pulses(d):
    """pulses [rel:]ON_DB:OFF_DB[:W[:minLen[:events=N]]] (additive, zeroSpan only): d['pulse.spec'] = dict(rel, on_db, off_db,
    W, min_len, capacity), or None when the key is off."""
    text = _key_text(d, "pulses", "pulse.spec", "pulsesSave")
    if not text:
        return
    spec = dict(rel=False, on_db=0.0, off_db=0.0, W=16, min_len=1, capacity=1024)
    try:
        parts = text.split(":")
        if parts[0].lower() == "rel":
            spec["rel"] = True
            parts = parts[1:]
        if not 2 <= len(parts) <= 5:
            raise ValueError(text)
        spec["on_db"], spec["off_db"] = float(parts[0]), float(parts[1])
        if len(parts) > 2:
            spec["W"] = int(parts[2])
        if len(parts) > 3:
            spec["min_len"] = int(parts[3])
        _options(parts[4:], spec, {"events": "capacity"})
        if not (np.isfinite(spec["on_db"]) and np.isfinite(spec["off_db"]) and spec["off_db"] <= spec["on_db"]
                and 1 <= spec["W"] <= _pulse.MAX_W and 1 <= spec["min_len"] <= _pulse.MAX_MIN_LEN
                and 1 <= spec["capacity"] <= _pulse.MAX_CAPACITY):
            raise ValueError(text)
        if not spec["rel"]:                      # the absolute levels are the library's: 0 < off <= on <= 4, thr_off >= 1
            on, off = _pulse.db_to_power(spec["on_db"]), _pulse.db_to_power(spec["off_db"])
            if not (0 < off <= on <= 4 and round(off * _pulse.POWER_UNIT * spec["W"]) >= 1):
                raise ValueError(text)
    except ValueError:
        _refuse(d, "pulses", text, PULSE_RULE)
    if _gate(d, "pulses", text):
        return
    if d["zoom"] or d["channels"]:
        prg_quit(d, "ERROR:handle_args: pulses [{}] reads the raw blocks: detecting pulses behind zoom or channels is out of scope, "
                    "drop [{}]".format(text, "zoom" if d["zoom"] else "channels"))
    d["pulse.spec"] = spec


IQFIX_RULE = ("iqfix wants MODE[:blocks=N][:track] with MODE dc|iq|dc+iq, an integer 1 <= N <= frameBatch blocks of the first batch "
              "that are measured (default: all of it), or track: every batch is measured and corrects the next; blocks= and track "
              "exclude each other")


def _handle_iqfix(d):
    """iqfix MODE[:blocks=N][:track] (additive, zeroSpan only): d['iqfix.spec'] = dict(mode, blocks, track), or None when the
    key is off; mode is the library's bits and blocks is None for all of the first batch."""
    text = _key_text(d, "iqfix", "iqfix.spec", "iqfixSave")
    if not text:
        return
    spec = dict(mode=0, blocks=None, track=False)
    try:
        parts = text.split(":")
        if parts[0] not in _iqfix.MODES:
            raise ValueError(text)
        spec["mode"] = _iqfix.MODES[parts[0]]
        for part in parts[1:]:
            name, eq, value = part.partition("=")
            if name == "track" and not eq and not spec["track"]:
                spec["track"] = True
            elif name == "blocks" and eq and spec["blocks"] is None:
                spec["blocks"] = int(value)
                if not 1 <= spec["blocks"] <= d["frameBatch"]:
                    raise ValueError(text)
            else:
                raise ValueError(text)
        if spec["track"] and spec["blocks"] is not None:
            raise ValueError(text)
    except ValueError:
        _refuse(d, "iqfix", text, IQFIX_RULE)
    if _gate(d, "iqfix", text, "the PSD diagnostic reads the raw block"):
        return
    for other in ("channels", "correlate", "pulses"):
        if d[other]:
            prg_quit(d, "ERROR:handle_args: iqfix [{}] corrects the blocks the engine and zoom read: {} [{}] reads the raw blocks, "
                        "drop either".format(text, other, d[other]))
    block_len = d["zoom.spec"]["block_len"] if d["zoom.spec"] is not None else d["fullSize"]
    if d["frameBatch"] * block_len > _iqfix.MAX_IN:
        prg_quit(d, "ERROR:handle_args: iqfix [{}]: frameBatch [{}] x [{}] samples per block exceed the corrector's [{}] per call".format(
            text, d["frameBatch"], block_len, _iqfix.MAX_IN))
    d["iqfix.spec"] = spec


DEMOD_PCM_SCALE = 32767.0                    # int16 per unit of the filtered detector: AM full scale 1, FM and PM one cycle
DEMOD_RULE = ("demod wants MODE[:audioDecim[:tapsPerPhase[:deemphUs]]] with MODE am|fm|pm, an integer 1 <= audioDecim <= %d, an "
              "integer tapsPerPhase >= 1 with audioDecim x tapsPerPhase <= %d and a finite deemphUs > 0 (defaults: audioDecim 1, "
              "tapsPerPhase 8, no de-emphasis); it needs zoom (zoom 1 passes the whole band) and a fullSize above "
              "audioDecim x tapsPerPhase" % (_demod.MAX_DECIM, _demod.MAX_TAPS))


def _handle_demod(d):
    """demod MODE[:audioDecim[:tapsPerPhase[:deemphUs]]] (additive, zeroSpan only, behind zoom): d['demod.spec'] =
    dict(mode, decim, taps_per_phase, ntaps, deemph_us, out_per_block, rate), or None when the key is off."""
    text = _key_text(d, "demod", "demod.spec", "demodSave")
    if not text:
        return
    try:
        parts = text.split(":")
        if not 1 <= len(parts) <= 4:
            raise ValueError(text)
        mode = parts[0].lower()
        decim = int(parts[1]) if len(parts) > 1 else 1
        tpp = int(parts[2]) if len(parts) > 2 else 8
        deemph = float(parts[3]) if len(parts) > 3 else None
        if not (mode in _demod.MODES and 1 <= decim <= _demod.MAX_DECIM and tpp >= 1 and decim * tpp <= _demod.MAX_TAPS
                and (deemph is None or (np.isfinite(deemph) and deemph > 0))):
            raise ValueError(text)
    except ValueError:
        _refuse(d, "demod", text, DEMOD_RULE)
    if _gate(d, "demod", text, "the PSD diagnostic sees the whole band"):
        return
    ntaps = decim * tpp
    lead = 1 if mode == "fm" else 0
    front = d["zoom.spec"] if d["zoom.spec"] is not None else d["chan.spec"]       # channels stands in for zoom
    if front is None or (d["fullSize"] < ntaps + lead and not d["continuous"]):
        _refuse(d, "demod", text, DEMOD_RULE)
    exact = d["samplingRate"] / (front["decim"] * decim)
    rate = int(round(exact))
    if rate != exact:
        print("WARN:handle_args: demod [{}]: the audio rate [{}] is not an integer, the WAV file says [{}]".format(text, exact, rate))
    # continuous: a call that takes the stream from N0 to N1 samples yields ceil(N1 / D) - ceil(N0 / D); this is the most of a block
    per_block = -(-d["fullSize"] // decim) if d["continuous"] else (d["fullSize"] - lead - ntaps) // decim + 1
    d["demod.spec"] = dict(mode=mode, decim=decim, taps_per_phase=tpp, ntaps=ntaps, deemph_us=deemph,
                           out_per_block=per_block, rate=rate)


RESAMPLE_RULE = ("audioRate wants HZ[:tapsPerPhase] with a whole HZ >= 1 and an integer tapsPerPhase >= 1 (default 8); it needs demod, "
                 "a whole audio rate samplingRate / (zoom D x audioDecim) in front of it, L / M = HZ over that rate, reduced, with "
                 "L <= %d, M <= %d and M <= %d L, at most %d taps per phase and %d taps in all, and a block long enough for one "
                 "output" % (_resamp.MAX_L, _resamp.MAX_M, _resamp.MAX_RATIO, _resamp.MAX_PHASE_TAPS, _resamp.MAX_TAPS))


def _handle_resample(d):
    """audioRate HZ[:tapsPerPhase] (additive, zeroSpan only, behind demod): d['resample.spec'] = dict(rate, rate_in, L, M,
    taps_per_phase, phase_taps, in_per_block, out_per_block), or None when the key is off."""
    text = _key_text(d, "audioRate", "resample.spec")
    if not text:
        return
    try:
        parts = text.split(":")
        if not 1 <= len(parts) <= 2:
            raise ValueError(text)
        hz = float(parts[0])
        tpp = int(parts[1]) if len(parts) > 1 else 8
        if not (np.isfinite(hz) and hz >= 1 and hz == int(hz) and tpp >= 1):
            raise ValueError(text)
    except ValueError:
        _refuse(d, "audioRate", text, RESAMPLE_RULE)
    if _gate(d, "audioRate", text):
        return
    dspec = d["demod.spec"]
    if dspec is None:
        prg_quit(d, "ERROR:handle_args: audioRate [{}] needs demod: {}".format(text, RESAMPLE_RULE))
    front = d["zoom.spec"] if d["zoom.spec"] is not None else d["chan.spec"]
    try:
        L, M = rate_ratio(d["samplingRate"] / (front["decim"] * dspec["decim"]), hz)
        P = len(resample_taps(L, M, tpp)) // L
    except KsaError as e:
        prg_quit(d, "ERROR:handle_args: audioRate [{}]: {}: {}".format(text, e, RESAMPLE_RULE))
    if d["continuous"]:                      # the most a block of the stream can yield; no output is dropped
        per_block = -(-dspec["out_per_block"] * L // M)
    else:
        per_block = -(-dspec["out_per_block"] * L // M) - -(-(P - 1) * L // M)
        if per_block < 1:
            _refuse(d, "audioRate", text, RESAMPLE_RULE)
    d["resample.spec"] = dict(rate=int(hz), rate_in=dspec["rate"], L=L, M=M, taps_per_phase=tpp, phase_taps=P,
                              in_per_block=dspec["out_per_block"], out_per_block=per_block)


def _handle_pfb(d):
    """pfbTaps P (additive): the polyphase front end.  fullSize becomes P*fftSize (P segments of fftSize samples per
    spectrum), `window` names the taper of the prototype; the within-block overlap and fold have nothing left to do.
    pfbSpectra K (additive, needs pfbTaps): the integrating polyphase spectrometer, fullSize (P+K-1)*fftSize."""
    taps, spectra = d["pfbTaps"], d["pfbSpectra"]
    if spectra < 0:
        prg_quit(d, "ERROR:handle_args: pfbSpectra [{}] must be 0 (off) or >= 1".format(spectra))
    if spectra and d["prgMode"] == "ZEROSPANPLAY":
        print("WARN:handle_args: pfbSpectra [{}] is ignored when playing saved spectra".format(spectra))
        d["pfbSpectra"] = spectra = 0
    if spectra and (taps < 1 or taps > _engine.PFB_MAX_TAPS):
        prg_quit(d, "ERROR:handle_args: pfbSpectra [{}] needs pfbTaps 1..{}".format(spectra, _engine.PFB_MAX_TAPS))
    if taps < 0 or taps > _engine.PFB_MAX_TAPS:
        prg_quit(d, "ERROR:handle_args: pfbTaps [{}] must be 0 (off) or 1..{}".format(taps, _engine.PFB_MAX_TAPS))
    if taps == 0:
        return
    if d["bUsePSD"]:
        prg_quit(d, "ERROR:handle_args: pfbTaps [{}] needs bUsePSD false: the PSD diagnostic has no polyphase form".format(taps))
    if d["curScanCumuMode"] == "PSD":
        prg_quit(d, "ERROR:handle_args: pfbTaps [{}] cannot be combined with curScanCumuMode PSD".format(taps))
    if d["prgMode"] == "ZEROSPANPLAY":
        print("WARN:handle_args: pfbTaps [{}] is ignored when playing saved spectra".format(taps))
        d["pfbTaps"] = 0
        return
    dflt = defaults()
    if d["curScanNonOverlap"] != dflt["curScanNonOverlap"] or d["curScanCumuMode"] != dflt["curScanCumuMode"]:
        print("WARN:handle_args: curScanNonOverlap [{}] and curScanCumuMode [{}] are unused with pfbTaps [{}]".format(
            d["curScanNonOverlap"], d["curScanCumuMode"], taps))
    d["fullSize"] = (taps + max(1, spectra) - 1) * d["fftSize"]


# ----------------------------------------------------------------------------------------- the additive keys of the scan modes
def _scan_key_text(d, key, spec_key, save):
    """_key_text for a scan-only key.  d[spec_key] exists only while the key is on: the zeroSpan keys leave a None, these leave
    nothing, so that a command line without them fills `d` as it always did."""
    text = _key_text(d, key, spec_key, save)
    if not text:
        del d[spec_key]
    return text


def _scan_gate(d, key, text):
    """Where a scan-only key may run: under scan, fmScan and quickFullScan, which are all prgMode SCAN by now."""
    if d["prgMode"] != "SCAN":
        prg_quit(d, "ERROR:handle_args: {} [{}] is scan only, prgMode is [{}]".format(key, text, d["prgMode"]))


SCAN_DETECT_RULE = ("scanDetect wants T:G:THR with integers 1 <= T <= %d training and 0 <= G <= %d guard cells on either side and a "
                    "finite threshold 0 <= THR <= 100 in dB, optionally followed by :mode=ca|go|so, :minWidth=W (1..fftSize), "
                    ":maxGap=K (0..%d), :events=E (1..%d), :edge=K and :dc=K (0..fftSize/2-1 bins each), each at most once; "
                    "fftSize %d..%d" % (_detect.MAX_TRAIN, _detect.MAX_GUARD, _detect.MAX_GAP, _detect.MAX_CAPACITY,
                                        _detect.MIN_NBINS, _detect.MAX_NBINS))


def _handle_scan_detect(d):
    """scanDetect T:G:THR[:mode=ca|go|so][:minWidth=W][:maxGap=K][:events=E][:edge=K][:dc=K] (additive, scan modes only):
    d['survey.spec'] = dict(train, guard, threshold, mode, min_width, max_gap, capacity, edge, dc); no such entry when the key
    is off."""
    text = _scan_key_text(d, "scanDetect", "survey.spec", "scanDetectSave")
    if not text:
        return
    n = d["fftSize"]
    spec = dict(train=0, guard=0, threshold=0.0, mode="ca", min_width=1, max_gap=0, capacity=4096, edge=0, dc=0)
    try:
        parts = text.split(":")
        if len(parts) < 3:
            raise ValueError(text)
        spec["train"], spec["guard"], spec["threshold"] = int(parts[0]), int(parts[1]), float(parts[2])
        _options(parts[3:], spec, {"mode": "mode", "minwidth": "min_width", "maxgap": "max_gap", "events": "capacity",
                                   "edge": "edge", "dc": "dc"})
        if not (1 <= spec["train"] <= _detect.MAX_TRAIN and 0 <= spec["guard"] <= _detect.MAX_GUARD
                and np.isfinite(spec["threshold"]) and 0 <= spec["threshold"] <= 100 and spec["mode"] in _detect.MODES
                and 1 <= spec["min_width"] <= n and 0 <= spec["max_gap"] <= _detect.MAX_GAP
                and 1 <= spec["capacity"] <= _detect.MAX_CAPACITY and _detect.MIN_NBINS <= n <= _detect.MAX_NBINS
                and 0 <= spec["edge"] <= n // 2 - 1 and 0 <= spec["dc"] <= n // 2 - 1):
            raise ValueError(text)
    except ValueError:
        _refuse(d, "scanDetect", text, SCAN_DETECT_RULE)
    _scan_gate(d, "scanDetect", text)
    d["survey.spec"] = spec


SCAN_TRACK_RULE = ("scanTrack wants GAP:SLOP with integers 0 <= GAP <= %d missing passes and 0 <= SLOP <= %d stitched bins, optionally "
                   "followed by :minRows=R (>= 1 passes), :minSpans=S (>= 1) and :events=E (1..%d, default 4096), each at most once"
                   % (_track.MAX_ROW_GAP, _track.MAX_NBINS, _track.MAX_CAPACITY))


def _handle_scan_track(d):
    """scanTrack GAP:SLOP[:minRows=R][:minSpans=S][:events=E] (additive, scan modes only, needs scanDetect):
    d['surveyTrack.spec'] = dict(row_gap, bin_slop, min_rows, min_spans, capacity); no such entry when the key is off."""
    text = _scan_key_text(d, "scanTrack", "surveyTrack.spec", "scanTrackSave")
    if not text:
        return
    spec = dict(row_gap=0, bin_slop=0, min_rows=1, min_spans=1, capacity=4096)
    try:
        parts = text.split(":")
        if len(parts) < 2:
            raise ValueError(text)
        spec["row_gap"], spec["bin_slop"] = int(parts[0]), int(parts[1])
        _options(parts[2:], spec, {"minrows": "min_rows", "minspans": "min_spans", "events": "capacity"})
        if not (0 <= spec["row_gap"] <= _track.MAX_ROW_GAP and 0 <= spec["bin_slop"] <= _track.MAX_NBINS
                and 1 <= spec["min_rows"] < 2 ** 31 and 1 <= spec["min_spans"] < 2 ** 31
                and 1 <= spec["capacity"] <= _track.MAX_CAPACITY):
            raise ValueError(text)
    except ValueError:
        _refuse(d, "scanTrack", text, SCAN_TRACK_RULE)
    _scan_gate(d, "scanTrack", text)
    if d.get("survey.spec") is None:
        prg_quit(d, "ERROR:handle_args: scanTrack [{}] links the emissions of scanDetect: give [scanDetect T:G:THR] as well".format(text))
    total = int((d["endFreq"] - d["startFreq"]) / d["samplingRate"]) * d["fftSize"]
    if total > _track.MAX_NBINS:
        prg_quit(d, "ERROR:handle_args: scanTrack [{}]: the stitched range of [{}] entries exceeds the linker's [{}] bins".format(
            text, total, _track.MAX_NBINS))
    d["surveyTrack.spec"] = spec


# in the order handle_args calls them: a handler reads the specs of the ones before it (channels zoom's, demod either's, ...)
_HANDLERS = (_handle_pfb, _handle_density, _handle_mask, _handle_continuous, _handle_zoom, _handle_channels, _handle_detect, _handle_demod,
             _handle_resample, _handle_correlate, _handle_pulses, _handle_track, _handle_measure, _handle_iqfix, _handle_scan_detect,
             _handle_scan_track)


def print_info(d):
    """K:953-963."""
    print("INFO: startFreq[{}] centerFreq[{}] endFreq[{}]".format(d["startFreq"], d["centerFreq"], d["endFreq"]))
    print("INFO: samplingRate[{}], gain[{}], bUsePSD[{}]".format(d["samplingRate"], d["gain"], d["bUsePSD"]))
    print("INFO: fullSize[{}], fftSize[{}], curScanCumuMode[{}], window[{}]".format(
        d["fullSize"], d["fftSize"], d["curScanCumuMode"], d["window"]))
    print("INFO: minAmp4Clip[{}], curScanNonOverlap[{}], scanRangeNonOverlap[{}], bScanRangeBaseDataIsRaw[{}]".format(
        d["minAmp4Clip"], d["curScanNonOverlap"], d["scanRangeNonOverlap"], d["bScanRangeBaseDataIsRaw"]))
    print("INFO: prgMode [{}], prgLoopCnt[{}], bPltLevels[{}],  bPltHeatMap[{}]".format(
        d["prgMode"], d["prgLoopCnt"], d["bPltLevels"], d["bPltHeatMap"]))
    print("INFO: xRes [{}], bGrid [{}], pltCompress [{}], pltCompressHM [{}]".format(
        d["xRes"], d["bGrid"], d["pltCompress"], d["pltCompressHM"]))
    print("INFO: source [{}], device [{}], iqFormat [{}], frameBatch [{}]".format(d["source"], d["device"], d["iqFormat"],
                                                                                d["frameBatch"]))
    if d["pfbTaps"] and d.get("pfbSpectra"):
        print("INFO: pfbTaps [{}] pfbSpectra [{}]: fullSize[{}] = (pfbTaps + pfbSpectra - 1) x fftSize, power, density; prototype sinc x window[{}]".format(
            d["pfbTaps"], d["pfbSpectra"], d["fullSize"], d["window"]))
    elif d["pfbTaps"]:
        print("INFO: pfbTaps [{}]: fullSize[{}] = pfbTaps x fftSize, prototype sinc x window[{}]".format(
            d["pfbTaps"], d["fullSize"], d["window"]))
    if d.get("continuous"):
        print("INFO: continuous [True]: the raw blocks are taken as one back-to-back stream and the stages run their stream forms "
              "(zoom, channels, demod, audioRate, correlate, pulses); the per-block counts below are the most a block can yield")
    if d.get("zoom.spec"):
        z = d["zoom.spec"]
        print("INFO: zoom [{}]: span [{}] Hz around [{}] Hz, bin width [{}] Hz, low-pass of [{}] taps, [{}] samples per frame".format(
            z["decim"], z["span"], z["center"], z["span"] / d["fftSize"], z["ntaps"], z["block_len"]))
    if d.get("chan.spec"):
        c = d["chan.spec"]
        print("INFO: channels [{}]: oversampling [{}], prototype of [{}] taps, channel [{}]: span [{}] Hz around [{}] Hz, bin width [{}] Hz, "
              "[{}] samples per frame".format(c["nchan"], c["oversample"], c["ntaps"], c["pick"], c["span"], c["center"],
                                              c["span"] / d["fftSize"], c["block_len"]))
    if d.get("demod.spec"):
        m = d["demod.spec"]
        print("INFO: demod [{}]: audio decimation [{}], low-pass of [{}] taps, de-emphasis [{}] us, [{}] samples per block at [{}] Hz; "
              "{}".format(m["mode"], m["decim"], m["ntaps"], m["deemph_us"], m["out_per_block"], m["rate"],
                          "the blocks are demodulated as one stream" if d.get("continuous") else
                          "each block is demodulated on its own and the blocks abut"))
    if d.get("resample.spec"):
        r = d["resample.spec"]
        print("INFO: audioRate [{}]: [{}] Hz -> [{}] Hz by L / M = [{}] / [{}], [{}] taps per phase, [{}] samples per block".format(
            r["rate"], r["rate_in"], r["rate"], r["L"], r["M"], r["phase_taps"], r["out_per_block"]))
    if d.get("survey.spec"):
        v = d["survey.spec"]
        print("INFO: scanDetect [{}]: CFAR [{}] over every tuned band, [{}] training and [{}] guard cells, [{}] dB, the sightings "
              "of overlapping bands joined per pass; edge [{}] and dc [{}] bins".format(
                  d["scanDetect"], v["mode"], v["train"], v["guard"], v["threshold"], v["edge"], v["dc"]))


# ------------------------------------------------------------------------------------------ SDR seam
def open_source(d):
    """d['source']: rtlsdr (needs pyrtlsdr) | synth | file:<raw capture: uint8 I,Q, or int8 / int16 I,Q under iqFormat s8 / s16>."""
    src = d["source"]
    if src == "synth":
        return sources.SyntheticSdr()
    if src.startswith("file:"):
        fmt = d["iqFormat"] if d["iqFormat"] in ("s8", "s16") else "u8"
        return sources.FileSdr(src[5:], d["samplingRate"], d["centerFreq"], iq_format=fmt)
    try:
        import rtlsdr
    except ImportError:
        prg_quit(d, "ERROR: source rtlsdr needs the pyrtlsdr package; use `source synth` or `source file:<capture>`")
    return rtlsdr.RtlSdr()


_reopen_source = None     # set by main(): how a failed source is re-opened (the reference calls rtlsdr.RtlSdr() again, K:305)


def _calc_startendfreq(centerFreq, samplingRate):
    """K:275-278."""
    return centerFreq - samplingRate / 2, centerFreq + samplingRate / 2


def sdr_info(sdr):
    """K:281-284 (sources without these attributes print what they have)."""
    print("INFO:Sdr:SupportedGains:", getattr(sdr, "valid_gains_db", None))
    print("INFO:Sdr:Bandwidth:", getattr(sdr, "bandwidth", None))
    print("INFO:Sdr:freqCorrection:", getattr(sdr, "freq_correction", None))


def sdr_setup(sdr, fC, fS, gain):
    """K:287-308, same signature: tune, discard 16Ki settle samples; on any failure close and re-open the source and
    report False.  Returns (sdr, bOk)."""
    try:
        sdr.sample_rate = fS
        sdr.center_freq = fC
        sdr.gain = gain
        bOk = True
        sdr.read_samples(16 * 1024)
    except Exception:
        print("WARN:SetupSDR:FAILED: fC[{}] fS[{}] gain[{}]".format(fC, fS, gain))
        try:
            sdr.close()
        except Exception:
            pass
        if _reopen_source is not None:
            sdr = _reopen_source()
        bOk = False
    print("SetupSDR:{}: fC[{}] fS[{}] gain[{}]".format(bOk, fC, fS, gain))
    return sdr, bOk


SDR_READ_UNIT = 2 ** 18   # K:311


def raw_format(d):
    """What sdr_read's `raw` wants for d['iqFormat'] and d['sdr']: False (complex64 from read_samples), True (uint8 I,Q from
    read_bytes) or "s8" / "s16" (int8 / int16 I,Q from read_iq) -- the raw forms only when the source can deliver them."""
    fmt = d.get("iqFormat")
    if fmt == "u8":
        return hasattr(d["sdr"], "read_bytes")
    if fmt in ("s8", "s16") and hasattr(d["sdr"], "read_iq"):
        return fmt
    return False


def raw_dtype(raw):
    """dtype and values per sample of the blocks sdr_read(..., raw) returns."""
    if raw in ("s8", "s16"):
        return sources.IQ_FORMATS[raw][0], 2
    return (np.dtype(np.uint8), 2) if raw else (np.dtype(np.complex64), 1)


def sdr_read(sdr, length, raw=False):
    """K:312-347, same signature (+ raw): one capture block in <= 2^18-sample reads.  Returns complex64, or -- raw=True and a
    source that can deliver bytes -- uint8 I,Q pairs, or -- raw "s8" / "s16" and a source with read_iq -- int8 / int16 I,Q
    pairs (the unpack then runs on the GPU)."""
    fixed = raw if raw in ("s8", "s16") and hasattr(sdr, "read_iq") else None
    raw = raw is True and hasattr(sdr, "read_bytes")
    parts, left = [], int(length)
    while left > 0:
        n = min(left, SDR_READ_UNIT)
        if n < SDR_READ_UNIT:
            want = int(2 ** np.ceil(np.log2(n)))      # K:343: the dongle only reads power-of-two sizes
        else:
            want = n
        if fixed:
            parts.append(np.asarray(sdr.read_iq(want, fixed), dtype=sources.IQ_FORMATS[fixed][0])[:2 * n])
        elif raw:
            parts.append(np.asarray(sdr.read_bytes(2 * want), dtype=np.uint8)[:2 * n])
        else:
            parts.append(np.asarray(sdr.read_samples(want))[:n].astype(np.complex64))
        left -= n
    return np.concatenate(parts) if len(parts) > 1 else parts[0]


def get_engine(d, scan_total=0, max_frames=1):
    """One engine per (geometry, mode) -- rebuilt when a GUI toggle or argument changes the key."""
    key = (d["fftSize"], d["fullSize"], d["curScanNonOverlap"], d["curScanCumuMode"], d["window"], d["gain"],
           d["minAmp4Clip"], d["xRes"], scan_total, d["scanRangeNonOverlap"], max_frames, d["device"], d.get("pfbTaps", 0), d.get("pfbSpectra", 0))
    if d.get("ksa.key") != key:
        if d.get("ksa.engine") is not None:
            d["ksa.engine"].close()
        if d.get("pfbTaps", 0):      # the polyphase front end: `window` names the prototype's taper, the fold is the engine's
            shape = dict(window=d["window"], pfb_taps=d["pfbTaps"], pfb_spectra=d.get("pfbSpectra", 0))
        else:
            shape = dict(window=d["theWin"], cumu_mode=d["curScanCumuMode"])
        d["ksa.engine"] = SpectrumEngine(
            d["fftSize"], full_size=d["fullSize"], non_overlap=d["curScanNonOverlap"],
            gain=d["gain"], min_amp=d["minAmp4Clip"], xres=d["xRes"],
            max_frames=max_frames, device=d["device"], scan_total_entries=scan_total,
            scan_non_overlap=d["scanRangeNonOverlap"], **shape)
        d["ksa.key"] = key
        if d.get("Fft.Adj") is not None:
            d["ksa.engine"].set_adj(d["Fft.Adj"], scan=bool(scan_total))
    return d["ksa.engine"]


def psd_crosscheck(d, samples, mag):
    """bUsePSD (K:350, K:374-384, README.rst:523-529) as a CPU-only DIAGNOSTIC next to the GPU result, never in
    place of it: matplotlib's Welch PSD of the same block (mlab.psd, the routine behind plt.psd at K:382: Fs = 2,
    two-sided, scale_by_freq, mean over segments) is compared with the device result at the strongest bin.  Under the
    magnitude folds (AVG / MAX / MIN / RAW) it is first converted back to this program's amplitude convention
    (|X| = sqrt(P * Fs * sum(w^2)), then 2*winAdj/N as K:391); under curScanCumuMode PSD the device folded the same Welch
    PSD, so `pxx` itself is compared with it.  `noverlap` is truncated to an int: the reference's own branch passes the
    float and raises TypeError under matplotlib >= 3.8 (tests/golden/psd_*.npz are runs of the reference with that one
    shim).  Stores d['psd.cur'] (the linear PSD, fftshifted) and d['psd.check'] = (bin_gpu, bin_psd, level_gpu_dB,
    level_psd_dB)."""
    from matplotlib import mlab
    n, win = d["fftSize"], np.asarray(d["theWin"], dtype=np.float64)
    x = np.asarray(samples)
    if x.dtype == np.uint8:
        x = sources.unpack(x, "u8")
    elif x.dtype == np.int8 or x.dtype == np.int16:
        x = sources.unpack(x, "s8" if x.dtype == np.int8 else "s16")
    pxx, _ = mlab.psd(x.astype(np.complex128), NFFT=n, window=win, noverlap=int(n * (1 - d["curScanNonOverlap"])))
    if d["curScanCumuMode"] == "PSD":      # the device folded the same Welch PSD: like is compared with like
        amp = pxx
    else:
        amp = np.sqrt(pxx * 2.0 * np.sum(win ** 2)) * 2.0 * (n / np.sum(win)) / n
    kg, kp = int(np.argmax(mag)), int(np.argmax(amp))
    with np.errstate(divide="ignore"):
        lg, lp = 10 * np.log10(mag[kg]) - d["gain"], 10 * np.log10(amp[kp]) - d["gain"]
    d["psd.cur"], d["psd.check"] = pxx, (kg, kp, float(lg), float(lp))
    print("DBUG:bUsePSD: peak bin gpu[{}] psd[{}] level gpu[{:.3f}] psd[{:.3f}] dB".format(kg, kp, lg, lp))


def sdr_curscan(d):
    """Drop-in for K:351-397: float64[fftSize], fftshifted -- linear magnitudes, or under curScanCumuMode PSD the linear
    Welch PSD (what K:383 returns under bUsePSD)."""
    samples = sdr_read(d["sdr"], d["fullSize"], raw=raw_format(d))
    mag = get_engine(d).curscan(samples)
    if d["bUsePSD"]:
        psd_crosscheck(d, samples, mag)
    return mag


_gpu_curscan = sdr_curscan   # zero_span fuses curscan + accumulate on the device while this is still bound


# ---------------------------------------------------------------------------------------- persistence
class _NumpyOnlyUnpickler(pickle.Unpickler):
    """The reference's save files are pickle streams of floats and float64 ndarrays (K:511-525, K:740-742).
    Only those reconstructors are admitted, so a crafted file cannot execute code."""
    _ok = {("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"),
           ("numpy", "ndarray"), ("numpy", "dtype"), ("numpy.core.multiarray", "scalar"),
           ("numpy._core.multiarray", "scalar"), ("numpy", "float64"),
           ("numpy.core.numeric", "_frombuffer"), ("numpy._core.numeric", "_frombuffer")}

    def find_class(self, module, name):
        if (module, name) in self._ok:
            return super().find_class(module, name)
        raise pickle.UnpicklingError("refusing %s.%s in a kspecanal save file" % (module, name))


def _load(f):
    return _NumpyOnlyUnpickler(f).load()


def _save_siglvls(d):
    """K:736-748."""
    if d["SaveSigLvls"] == "":
        return
    try:
        with open(d["SaveSigLvls"], "wb+") as f:
            pickle.dump(d["startFreq"], f)
            pickle.dump(d["endFreq"], f)
            pickle.dump(np.asarray(d["Fft.Avg"], dtype=np.float64), f)
        print("INFO:_save_siglvls: success...", d["SaveSigLvls"])
    except Exception:
        print("WARN:_save_siglvls: Failed...", d["SaveSigLvls"])


def _load_siglvls(d):
    """K:751-768: the saved range must match exactly, otherwise the adjustment is dropped."""
    d["Fft.Adj"] = None
    if d["AdjSigLvls"] == "":
        return
    try:
        with open(d["AdjSigLvls"], "rb") as f:
            start, end, adj = _load(f), _load(f), _load(f)
        if start == d["startFreq"] and end == d["endFreq"]:
            d["Fft.Adj"] = np.asarray(adj, dtype=np.float64)
            print("INFO:_load_siglvls: success...", d["AdjSigLvls"])
        else:
            print("ERRR:_load_siglvls:{}:savedRange[{}-{}] curFreqRange[{}-{}]".format(
                d["AdjSigLvls"], start, end, d["startFreq"], d["endFreq"]))
            d["AdjSigLvls"] = ""
    except Exception:
        print("WARN:_load_siglvls: Failed...", d["AdjSigLvls"])
        d["AdjSigLvls"] = ""


def _adj_siglvls(d, cur):
    """K:400-411: the curves are stored raw and adjusted on the way to the plot."""
    adj = d.get("Fft.Adj")
    if d["AdjSigLvls"] != "" and adj is not None:
        sub = lambda v: None if v is None else v - adj                      # (a curve switched off is still None, K:471-476)
        return sub(d["Fft.Max"]), sub(d["Fft.Min"]), sub(d["Fft.Avg"]), sub(cur)
    return d["Fft.Max"], d["Fft.Min"], d["Fft.Avg"], cur


# ------------------------------------------------------------------------------------------- plotting
def plt_figures(d):
    """K:1077-1115 reduced to what the hand-off needs: a Levels axes and a Heatmap axes.  Skipped entirely
    when both plots are off (headless runs, the GPU box)."""
    d["plt"] = None
    if not (d["bPltLevels"] or d["bPltHeatMap"]):
        return
    import matplotlib.pyplot as plt
    plt.ion()
    fig = plt.figure("kSpecAnal", figsize=(12, 8), constrained_layout=True)
    gs = fig.add_gridspec(nrows=16, ncols=5)
    d["AxLevels"] = fig.add_subplot(gs[:8, :4])
    d["AxFreqs"] = fig.add_subplot(gs[:8, 4])
    d["AxHeatMap"] = fig.add_subplot(gs[8:16, :4])
    d["AxFreqs"].set_xticks([])
    d["AxFreqs"].set_yticks([])
    d["plt"] = plt


def _plotcompress(d, data, mode):
    """K:168-202 for the plot side (host arrays are tiny here: <= totalEntries floats)."""
    if mode == "RAW" or len(data) // d["xRes"] == 0:
        return data
    if mode == "CONV":
        conv = np.kaiser(128, 64)                                  # K:87
        out = np.convolve(data, conv, mode="same")
        avg = np.average(out)
        out[:12] = avg
        out[-12:] = avg
        return out
    t = np.asarray(data).reshape(d["xRes"], len(data) // d["xRes"])
    if mode == "MAX":
        return t.max(axis=1)
    if mode == "MIN":        # unreachable in the reference (K:188 vs K:196); implemented as documented there
        return t.min(axis=1)
    return np.average(t, axis=1)


_data_plotcompress = _plotcompress     # the reference's name (K:168-202)


def data_plotcompress(d, x, y, mode=None):
    """K:205-221."""
    mode = d["pltCompress"] if mode is None else mode
    if mode == "RAW":
        return x, y
    if mode == "CONV":
        return x, _plotcompress(d, y, mode)
    return _plotcompress(d, x, "AVG"), _plotcompress(d, y, mode)


def data_2d_plotcompress(d, data, mode=None):
    """K:224-237: every row of a 2-D set reduced like _data_plotcompress (the reference uses it once, to build the scan's
    initial waterfall buffer at K:614; the engine's rings are born decimated, so this is the host-side name for callers
    that hold full-width rows)."""
    mode = d["pltCompressHM"] if mode is None else mode
    if mode == "RAW":
        return data
    return np.array([_plotcompress(d, np.asarray(data)[r, :], mode) for r in range(np.asarray(data).shape[0])])


def plot_highs(d, freqs, levels, eng=None, curve=None, scan=False):
    """K:243-272: the strongest points of the last plotted curve, at least pltHighsDelta4Marking of the span apart.
    With an engine the selection runs on the device over the same decimated curve (ksa_read_highs) and only the
    marked cells come back; otherwise (RAW / CONV curves that are on the host anyway) the same walk runs here:
    descending argsort, the lowest point never visited (K:258).  Returns the list of (freq, level)."""
    delta = d["pltHighsDelta4Marking"] * (freqs[-1] - freqs[0])
    count = d["pltHighsNumMarkers"]
    marked = []
    if eng is not None and curve is not None and 1 <= count <= 64 and len(freqs) > 1:
        cell = (freqs[-1] - freqs[0]) / (len(freqs) - 1)
        idx, lvl = eng.highs(len(freqs), d["pltCompress"], curve, min_sep=delta / cell, count=count, scan=scan)
        marked = [(float(freqs[i]), float(v)) for i, v in zip(idx, lvl)]
    else:
        order = np.argsort(levels)
        for j in range(1, len(freqs)):
            i = order[-j]
            if all(abs(freqs[i] - f) >= delta for f, _ in marked):
                marked.append((float(freqs[i]), float(levels[i])))
                if len(marked) >= count:
                    break
    _show_highs(d, marked)
    return marked


def _view_on_device(d, n):
    """The Levels curves can be decimated on the device (pltCompress AVG|MAX|MIN over whole groups, K:186-201): then
    only xRes-sized arrays have to cross PCIe per frame / pass."""
    return d["pltCompress"] in ("AVG", "MAX", "MIN") and n // d["xRes"] > 0 and n % d["xRes"] == 0


def _materialize(d, eng, scan=False):
    """The FULL-width hand-off arrays d['Fft.Cur'|'Fft.Max'|'Fft.Min'|'Fft.Avg'] and the whole [128, W] waterfall
    buffer, read from the device: on demand (RAW / CONV Levels plots, K:205-221), and once when a run ends
    (SaveSigLvls K:736-748, callers of main())."""
    st = eng.scan_state() if scan else eng.state()
    for k in ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg"):
        d[k] = st[k]
    if not scan:
        for flag, k in (("bDataMax", "Fft.Max"), ("bDataMin", "Fft.Min"), ("bDataAvg", "Fft.Avg")):
            if not d[flag]:
                d[k] = None                                                 # still None in the reference, K:471-476
    d["fftHM"], d["fftHMIndex"] = st["fftHM"], st["hm_index"]
    d["handoff.bytes"] = sum(st[k].size for k in ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg", "fftHM")) * 4
    return st


def _handoff(d, eng, freqs, scan=False, new_rows=1):
    """What one frame (zeroSpan, K:477-504) or one pass (scan, K:669-697 + K:729) hands to the plots.  With a
    decimating pltCompress everything is reduced on the device and ONE call (ksa_read_view) brings back the four
    xRes-point curves, the peak markers of the last plotted curve and the one new waterfall row: 4*xRes + xRes
    floats instead of 4*N + 128*W.  RAW / CONV plots need the full curves and materialise them.  After a batch of
    frames (frameBatch) the newest `new_rows` (<= 128) ring rows come back in the same call."""
    if not _view_on_device(d, len(freqs)):
        _materialize(d, eng, scan)
        _plot_heatmap(d, d["fftHM"])
        _plot_levels(d, freqs, d["Fft.Cur"])
        return
    last = None
    for flag in ("bDataMax", "bDataMin", "bDataAvg", "bDataCur"):        # plotting order of K:489-503: the last one is marked
        if d[flag]:
            last = flag[5:].lower()
    # decimated x axis, cached by VALUE of the axis (an id() of a freed array can come back for a different axis)
    key = (len(freqs), float(freqs[0]), float(freqs[-1]), d["xRes"])
    if d.get("Levels.key") != key:
        d["Levels.x"], d["Levels.key"] = _plotcompress(d, freqs, "AVG"), key
    xs = d["Levels.x"]
    count = d["pltHighsNumMarkers"]
    cell = (xs[-1] - xs[0]) / (len(xs) - 1) if len(xs) > 1 else 1.0
    delta = d["pltHighsDelta4Marking"] * (xs[-1] - xs[0])
    want_marks = last is not None and 1 <= count <= 64 and len(xs) > 1
    lv, idx, lvl, rows, hm_index = eng.view(d["xRes"], d["pltCompress"], curve=last if want_marks else None,
                                            min_sep=delta / cell, count=count, hm_rows=new_rows, scan=scan)
    d["handoff.bytes"] = (lv.size + rows.size + 2 * len(idx)) * 4
    d["Levels"] = {"x": xs, "max": lv[1], "min": lv[2], "avg": lv[3], "cur": lv[0]}
    for r in range(new_rows):                                             # the host copy of the ring takes the new rows (K:480 / K:697)
        d["fftHM"][(hm_index - new_rows + r) % _engine.HM_ROWS] = rows[r]
    d["fftHMIndex"] = hm_index
    _plot_heatmap(d, d["fftHM"])
    drawing = d.get("plt") is not None and d["bPltLevels"]
    if drawing:
        d["AxLevels"].cla()
        if d["bGrid"]:
            d["AxLevels"].grid(True)
        for flag, row, colour in (("bDataMax", 1, "r"), ("bDataMin", 2, "y"), ("bDataAvg", 3, "g"), ("bDataCur", 0, "b")):
            if d[flag]:
                d["AxLevels"].plot(xs, lv[row], colour)
    if last is not None:
        if want_marks:
            _show_highs(d, [(float(xs[i]), float(v)) for i, v in zip(idx, lvl)])
        else:     # more markers than the device kernel returns (64), or a one-point curve: the host walk over the decimated curve
            plot_highs(d, xs, lv[{"cur": 0, "max": 1, "min": 2, "avg": 3}[last]])


def _show_highs(d, marked):
    """The drawing half of plot_highs (K:263-267)."""
    d["Highs"] = marked
    if d.get("plt") is not None and d["bPltLevels"]:
        d["AxFreqs"].clear()
        d["AxFreqs"].set_xticks([])
        d["AxFreqs"].set_yticks([])
        for n, (f, lvl) in enumerate(marked):
            d["AxLevels"].plot(f, lvl, "o", label=f)
            d["AxFreqs"].text(0.1, 1.0 - 0.1 * (n + 1), "{}:{}".format(round(f / 1e6, 8), round(lvl, 2)))


def _plot_levels(d, freqs, cur):
    """Levels hand-off from FULL host arrays (K:485-504 / K:670-688): the RAW / CONV modes, which plot every bin."""
    fmax, fmin, favg, fcur = _adj_siglvls(d, cur)
    x = y = None
    curves = (("bDataMax", fmax, "r"), ("bDataMin", fmin, "y"), ("bDataAvg", favg, "g"), ("bDataCur", fcur, "b"))
    if d.get("plt") is not None and d["bPltLevels"]:
        d["AxLevels"].cla()
        if d["bGrid"]:
            d["AxLevels"].grid(True)
    for flag, data, colour in curves:
        if d[flag] and data is not None:
            x, y = data_plotcompress(d, freqs, data)
            if d.get("plt") is not None and d["bPltLevels"]:
                d["AxLevels"].plot(x, y, colour)
    if x is not None:
        plot_highs(d, x, y)


def _plot_heatmap(d, hm):
    if d.get("plt") is None or not d["bPltHeatMap"]:
        return
    if d.get("hm.artist") is None:
        d["hm.artist"] = d["AxHeatMap"].imshow(hm, extent=(0, 1, 0, 1), aspect="auto", interpolation="bicubic")
        d["AxHeatMap"].set_xticks([0, 0.25, 0.5, 0.75, 1])
        d["AxHeatMap"].set_xticklabels([d["startFreq"], (d["startFreq"] + d["centerFreq"]) / 2, d["centerFreq"],
                                        (d["centerFreq"] + d["endFreq"]) / 2, d["endFreq"]])
    d["hm.artist"].set_data(hm)                                    # K:481 / K:729
    d["hm.artist"].autoscale()
    d["plt"].pause(0.0001)


# ------------------------------------------------------------------------------------------ zeroSpan
def zero_span(d):
    """K:426-505.  Per frame: capture, curscan + LogNoGain + Max/Min/Avg/Cur + waterfall row on the GPU,
    then the hand-off arrays are refreshed for the plots.  Every additive key that is on is a stage (_STAGES) beside that."""
    for k in ("Fft.Max", "Fft.Min", "Fft.Avg", "Fft.Cur"):
        d[k] = None
    d["timeWasStr"] = None
    if d.get("sdr") is not None:
        d["sdr"], _ = sdr_setup(d["sdr"], d["centerFreq"], d["samplingRate"], d["gain"])
    fused = sdr_curscan is _gpu_curscan          # not playback: only then are there blocks for the stages and for batches
    specs = {key: d.get(key) for key, _ in _STAGES} if fused else {}
    front = specs.get("zoom.spec") or specs.get("chan.spec")     # either front end: the decimated rate around its centre
    if front is None:
        specs.pop("demod.spec", None)            # the demodulator reads a front end's blocks
        freqs = np.fft.fftshift(np.fft.fftfreq(d["fftSize"], 1 / d["samplingRate"]) + d["centerFreq"])   # K:444-445
    else:                                        # the zoomed span: the decimated rate around the mixer's frequency
        freqs = np.fft.fftshift(np.fft.fftfreq(d["fftSize"], front["decim"] / d["samplingRate"]) + front["center"])
    d["freqs"] = freqs
    print("ZeroSpan: min[{}] max[{}]".format(min(freqs), max(freqs)))
    batch = d["frameBatch"]
    if batch > 1 and not fused:
        print("WARN:zero_span: frameBatch [{}] is ignored when playing saved spectra".format(batch))
        batch = 1
    eng = get_engine(d, max_frames=batch)
    eng.reset()
    d["fftHM"], d["fftHMIndex"] = np.zeros((_engine.HM_ROWS, eng.hm_width)), 0     # K:456; the device ring starts the same
    raw = raw_format(d) if fused else False
    run = _Run(batch, front["block_len"] if front is not None else d["fullSize"], raw, _raw_fmt(raw), front, freqs)
    stages = []                                  # in the order of _STAGES, which is the order of the hand-off
    try:
        for key, cls in _STAGES:
            if specs.get(key) is not None:
                stages.append(cls(d, specs[key], run))
        # every stage runs the batch route: frameBatch 1 is a batch of one; so does continuous, whose reader lives there
        if stages or batch > 1 or (fused and d.get("continuous")):
            _zero_span_batches(d, eng, run, stages)
        else:
            _zero_span_frames(d, eng, freqs)
        for stage in stages:
            stage.handoff(d)
    finally:
        for stage in reversed(stages):           # every object owns its buffers and its destroy drains the stream first
            stage.close()
    if _materialize(d, eng)["frames"] == 0:      # full-width arrays once, for SaveSigLvls and whoever called main()
        for k in ("Fft.Max", "Fft.Min", "Fft.Avg", "Fft.Cur"):
            d[k] = None                          # no frame ran: the curves are still None (K:427-430)


_Run = collections.namedtuple("_Run", "batch block_len raw fmt front freqs")
_Run.__doc__ = """What zero_span tells every stage about the run: the batch size, the samples of one raw block, what sdr_read's `raw`
wants and the FMT_* of such blocks, the spec of the front end (zoom or channels) or None, and the frequency axis."""


def _raw_fmt(raw):
    """The FMT_* of the blocks sdr_read(..., raw) returns."""
    return {False: FMT_C64, True: FMT_U8, "s8": FMT_S8, "s16": FMT_S16}[raw]


# A stage is the state of one additive key over a zeroSpan run: __init__(d, spec, run), one feeding method whose name tells
# _zero_span_batches where it stands (feed_raw | front | feed | feed_rows), handoff(d) and close().
class _DensityFeed:
    """The density key's state over a run: the SpectrumDensity, fed every batch's dB rows; its columns are the waterfall's."""

    def __init__(self, d, spec, run):
        self.dens = SpectrumDensity(d["fftSize"], d["ksa.engine"].hm_width, spec[0], spec[1], spec[2], device=d["device"])

    def feed_rows(self, db):
        self.dens.add_rows(db)

    def handoff(self, d):
        """The density's hand-off arrays (drawing the bitmap is the caller's: density.image), the INFO line, densitySave."""
        dens = self.dens
        counts, rows = dens.read()
        levels = dens.levels
        d["density"], d["densityNaN"] = counts[:levels], counts[levels]
        d["densityEdges"], d["densityRows"] = dens.level_edges(), rows
        total = int(counts.sum())
        clamped = int(counts[0].sum()) + (int(counts[levels - 1].sum()) if levels > 1 else 0)
        print("INFO:zero_span: density rows [{}], levels [{}] x columns [{}], share of counts in the two clamped levels [{:.6f}]".format(
            rows, levels, dens.width, clamped / total if total else 0.0))
        if d["densitySave"]:
            with open(d["densitySave"], "wb") as f:
                np.save(f, counts)                   # [L+1, W] int64, the NaN row last

    def close(self):
        self.dens.close()


class _MaskFeed:
    """The mask key's state over a run: the SpectrumMask (made at once for flat / file, after the first F frames for learn),
    the rows being learnt from, and the dB spectra of the stored events, picked from each batch's rows as the events arrive."""

    def __init__(self, d, spec, run):
        self.spec, self.n, self.device = spec, d["fftSize"], d["device"]
        self.mask, self.learnt, self.frames_done = None, [], 0
        self.event_rows, self.stored = [], 0
        if spec["kind"] != "learn":
            self._make(spec["upper"], spec["lower"])

    def _make(self, upper, lower):
        self.mask = SpectrumMask(self.n, upper, lower, min_bins=self.spec["min_bins"], capacity=self.spec["capacity"],
                                 device=self.device)

    def feed_rows(self, db):
        """db: float32 [k][fftSize], the dB rows of frames frames_done .. frames_done + k of the run."""
        first = self.frames_done
        self.frames_done += len(db)
        if self.mask is None:                        # learn:F:M -- the boundary may fall inside a batch
            take = min(len(db), self.spec["frames"] - first)
            self.learnt.append(np.array(db[:take], dtype=np.float32))
            if first + take < self.spec["frames"]:
                return
            self._make(learn_mask(np.concatenate(self.learnt), self.spec["margin"]), None)
            self.mask.set_row_base(self.spec["frames"])  # row numbers are frame numbers of the run
            self.learnt = []
            db, first = db[take:], first + take
        if not len(db):
            return
        self.mask.check_rows(db)
        if self.stored < self.mask.capacity:
            ev, _ = self.mask.events()
            for row in ev["row"][self.stored:]:
                self.event_rows.append(np.array(db[row - first], dtype=np.float32))
            self.stored = len(ev)

    def handoff(self, d):
        """The hand-off arrays, the INFO line, maskSave."""
        n = self.n
        rows_arr = np.array(self.event_rows, dtype=np.float32).reshape(-1, n)
        if self.mask is None:
            print("WARN:zero_span: mask learn wanted [{}] frames, the run had [{}]: nothing was checked".format(
                self.spec["frames"], self.frames_done))
            ev, total, hits, rows = np.zeros(0, dtype=EVENT_DTYPE), 0, np.zeros((3, n), dtype=np.int64), 0
            upper, lower = np.full(n, np.inf, dtype=np.float32), np.full(n, -np.inf, dtype=np.float32)
            busiest, share = -1, 0.0
        else:
            ev, total = self.mask.events()
            hits, rows = self.mask.hits()
            upper = self.mask.upper
            lower = np.full(n, -np.inf, dtype=np.float32) if self.mask.lower is None else self.mask.lower
            occ = self.mask.occupancy()
            busiest = int(np.argmax(occ))
            share = float(occ[busiest])
        d["maskEvents"], d["maskEventsTotal"], d["maskHits"], d["maskRows"], d["maskEventRows"] = ev, total, hits, rows, rows_arr
        print("INFO:zero_span: mask rows [{}], events stored [{}] / total [{}], highest occupancy [{:.6f}] at bin [{}]".format(
            rows, len(ev), total, share, busiest))
        if d["maskSave"]:
            with open(d["maskSave"], "wb") as f:
                np.savez(f, events=ev, events_total=np.int64(total), hits=hits, rows_seen=np.int64(rows), upper=upper,
                         lower=lower, event_rows=rows_arr)

    def close(self):
        if self.mask is not None:
            self.mask.close()


class _DetectFeed:
    """The detect key's state over a run: the SignalDetector, fed every batch's dB rows; row numbers are frame numbers."""

    def __init__(self, d, spec, run):
        self.spec, self.freqs = spec, run.freqs
        # one row is one frame: fullSize samples at the rate the engine was fed
        self.row_period_s = d["fullSize"] * (run.front["decim"] if run.front is not None else 1) / d["samplingRate"]
        self.det = SignalDetector(d["fftSize"], spec["train"], spec["guard"], spec["threshold"], mode=spec["mode"],
                                  min_width=spec["min_width"], max_gap=spec["max_gap"], capacity=spec["capacity"],
                                  device=d["device"])
        # the measure key: a meter whose result i belongs to the detector's emission i
        self.plan, self.meter, self.measured = d.get("measure.plan"), None, 0
        if self.plan is not None:
            try:
                self.meter = SpectrumMeter(d["fftSize"], capacity=spec["capacity"], occupied=self.plan["occupied"],
                                           xdb=self.plan["xdb"], margin=self.plan["margin"], device=d["device"])
            except Exception:
                self.det.close()
                raise

    def feed_rows(self, db):
        """db: float32 [k][fftSize], the dB rows of the run's next k frames."""
        if not len(db):
            return
        if self.meter is None:
            self.det.detect_rows(db)
            return
        base = self.det.rows_seen
        self.det.detect_rows(db)
        # the batch's rows against the detector's buffer where it lies, from the emissions stored before the batch
        self.meter.measure_detector(self.det, np.asarray(db, dtype=np.float32), row_base=base, first=self.measured)
        self.measured = SpectrumMeter.detector_list(self.det)[3]

    def handoff(self, d):
        """The hand-off arrays, the INFO line, detectSave; then, with the track key, the link over these emissions."""
        ev, total = self.det.emissions()
        hits, rows = self.det.hits()
        occ = self.det.occupancy()
        busiest = int(np.argmax(occ))
        d["detectEmissions"], d["detectEmissionsTotal"], d["detectHits"], d["detectRows"] = ev, total, hits, rows
        print("INFO:zero_span: detect rows [{}], emissions stored [{}] / total [{}], highest occupancy [{:.6f}] at bin [{}]".format(
            rows, len(ev), total, float(occ[busiest]), busiest))
        if d["detectSave"]:
            center, width = emission_freqs(ev, self.freqs)
            s = self.spec
            with open(d["detectSave"], "wb") as f:
                np.savez(f, emissions=ev, emissions_total=np.int64(total), hits=hits, rows_seen=np.int64(rows),
                         train=np.int32(s["train"]), guard=np.int32(s["guard"]), threshold_db=np.float32(s["threshold"]),
                         mode=np.array(s["mode"]), min_width=np.int32(s["min_width"]), max_gap=np.int32(s["max_gap"]),
                         center_hz=center, width_hz=width)
        if self.meter is not None:
            self.measure_handoff(d, ev)
        if d.get("track.spec") is not None:
            self.link(d)

    def measure_handoff(self, d, ev):
        """The measure key: the results of the stored emissions `ev`, the INFO line, measureSave."""
        res = self.meter.results(0, len(ev))
        d["measureResults"] = res
        done = (res["flags"] & _measure.FLAG_MEASURED) != 0
        obw = (res["obw_hi"] - res["obw_lo"] + 1)[done & (res["nvalid"] > 0)]
        print("INFO:zero_span: measure spans measured [{}] / emissions [{}], median OBW [{}] bins, strongest power [{:.2f}] dB".format(
            int(done.sum()), len(ev), float(np.median(obw)) if len(obw) else 0.0,
            float(res["power_db"][done].max()) if done.any() else float("-inf")))
        if d["measureSave"]:
            width = (res["bin_hi"] - res["bin_lo"] + 1).astype(np.float64)
            noise = width * np.power(10.0, ev["floor_db"].astype(np.float64) / 10.0)      # the floor over the window summed
            net = np.where(done, res["power"] - noise, np.nan)
            with np.errstate(invalid="ignore", divide="ignore"):
                net_db = np.where(net > 0, 10.0 * np.log10(np.where(net > 0, net, 1.0)), np.nan)
                snr_db = np.where((net > 0) & (noise > 0), 10.0 * np.log10(np.where(net > 0, net, 1.0) / np.where(noise > 0, noise, 1.0)),
                                  np.nan)
            p = self.plan
            with open(d["measureSave"], "wb") as f:
                np.savez(f, results=res, occupied_percent=np.float64(p["percent"]), occupied=np.float32(p["occupied"]),
                         xdb=np.float32(p["xdb"]), margin=np.int32(p["margin"]), power_net_db=net_db, snr_db=snr_db,
                         **result_freqs(res, self.freqs))

    def link(self, d):
        """The track key: one link over the detector's whole buffer where it lies; the hand-off arrays, the INFO line,
        trackSave."""
        s, freqs, row_period_s = d["track.spec"], self.freqs, self.row_period_s
        trk = EmissionTracker(d["fftSize"], row_gap=s["row_gap"], bin_slop=s["bin_slop"], min_rows=s["min_rows"],
                              min_spans=s["min_spans"], capacity=s["capacity"], max_spans=self.det.capacity, device=d["device"])
        try:
            trk.link_detector(self.det)
            tr, total, comps = trk.tracks()
            labels = trk.labels()
        finally:
            trk.close()
        d["trackTracks"], d["trackTotal"], d["trackComponents"], d["trackLabels"] = tr, total, comps, labels
        longest = int((tr["row_last"] - tr["row_first"] + 1).max()) if len(tr) else 0
        print("INFO:zero_span: track emissions [{}], components [{}], tracks stored [{}] / total [{}], longest [{}] rows, open at the end [{}]".format(
            len(labels), comps, len(tr), total, longest, int(np.count_nonzero(tr["flags"] & _track.FLAG_OPEN_END))))
        if d["trackSave"]:
            with open(d["trackSave"], "wb") as f:
                np.savez(f, tracks=tr, tracks_total=np.int64(total), components_total=np.int64(comps), labels=labels,
                         row_gap=np.int32(s["row_gap"]), bin_slop=np.int32(s["bin_slop"]), min_rows=np.int32(s["min_rows"]),
                         min_spans=np.int32(s["min_spans"]), capacity=np.int32(s["capacity"]),
                         row_period_s=np.float64(row_period_s), **track_times_freqs(tr, freqs, row_period_s))

    def close(self):
        if self.meter is not None:
            self.meter.close()
        self.det.close()


def _gather_events(feed, obj, got):
    """What _CorrFeed and _PulseFeed do after a batch of `got` blocks went to their object: the events that are new are kept
    with `block` counted over the run, not over the batch; where the object's list is full there is nothing to fetch.  The
    records of the stream form (feed.stream) stay as they are: block -1, positions counted over the stream."""
    if feed.stored < obj.capacity:
        ev = obj.events()[0]                         # synchronises: the buffer is free for the next batch
        new = ev[feed.stored:]
        if not feed.stream:
            new["block"] += feed.blocks_done
        feed.parts.append(new)
        feed.stored = len(ev)
    else:
        obj.synchronize()
    feed.blocks_done += got


class _CorrFeed:
    """The correlate key's state over a run: the Correlator, whose block form runs over every batch's raw blocks in their
    iqFormat, read from the page-locked batch buffer; block numbers are frame numbers of the run.  Under continuous the stream
    form runs over the batch as one piece of the stream (kcr_process_dev, kcr_flush at the hand-off): block is -1 and pos
    counts from the run's first sample."""

    def __init__(self, d, spec, run):
        self.spec, self.full, self.rate, self.stream = spec, d["fullSize"], d["samplingRate"], bool(d.get("continuous"))
        self.corr = Correlator(spec["templates"], threshold=spec["threshold"], guard=spec["guard"], capacity=spec["capacity"],
                               max_in=run.batch * self.full, fmt=run.fmt, device=d["device"])
        self.blocks_done, self.stored, self.parts = 0, 0, []

    def feed_raw(self, blocks, got):
        """blocks: the batch buffer, whose first `got` rows are the run's next blocks."""
        if self.stream:                              # the first `got` rows of the batch buffer are contiguous
            self.corr.process_dev(blocks, got * self.full)
        else:
            self.corr.blocks_dev(blocks, got, self.full)
        _gather_events(self, self.corr, got)

    def handoff(self, d):
        """The hand-off arrays, the INFO line, correlateSave.  The stream form first decides the lags still pending."""
        if self.stream:
            self.corr.flush()
            _gather_events(self, self.corr, 0)
        _, total = self.corr.events()
        ev = np.concatenate(self.parts) if self.parts else np.zeros(0, dtype=_corr.EVENT_DTYPE)
        d["corrEvents"], d["corrTotal"] = ev, total
        best = float(ev["metric"].max()) if len(ev) else 0.0
        print("INFO:zero_span: correlate blocks [{}], templates [{}] of [{}] samples, events stored [{}] / total [{}], best metric [{:.6f}]".format(
            self.blocks_done, self.corr.Q, self.corr.K, len(ev), total, best))
        if d["correlateSave"]:
            frac = refine(ev)
            toa = np.stack([ev["block"].astype(np.float64), frac, frac / self.rate], axis=1).reshape(-1, 3)
            s = self.spec
            with open(d["correlateSave"], "wb") as f:
                np.savez(f, events=ev, events_total=np.int64(total), toa=toa, templates=s["templates"],
                         threshold=np.float32(s["threshold"]), guard=np.int32(s["guard"]), capacity=np.int32(s["capacity"]),
                         sampling_rate=np.float64(self.rate), block_len=np.int64(self.full),
                         **({"continuous": np.bool_(True)} if self.stream else {}))   # toa: -1, stream position, seconds in

    def close(self):
        self.corr.close()


class _PulseFeed:
    """The pulses key's state over a run: the PulseDetector, whose block form runs over every batch's raw blocks in their
    iqFormat, read from the page-locked batch buffer; block numbers are frame numbers of the run.  With rel: the levels are set
    from the median envelope of the run's first block before any block is searched.  Under continuous the stream form runs over
    the batch as one piece of the stream (kpl_process_dev, kpl_flush at the hand-off): a pulse across a block edge is one
    record, block is -1 and start counts from the run's first sample; rel: still measures the first block with the block form,
    which does not touch the stream's state."""

    def __init__(self, d, spec, run):
        self.spec, self.full, self.rate, self.stream = spec, d["fullSize"], d["samplingRate"], bool(d.get("continuous"))
        on, off = (1.0, 1.0) if spec["rel"] else (_pulse.db_to_power(spec["on_db"]), _pulse.db_to_power(spec["off_db"]))
        self.det = PulseDetector(W=spec["W"], on_power=on, off_power=off, min_len=spec["min_len"], capacity=spec["capacity"],
                                 max_in=run.batch * self.full, fmt=run.fmt, device=d["device"])
        self.floor = None                            # rel: the median of S / W over the first block, in units of 2^-30
        self.blocks_done, self.stored, self.parts = 0, 0, []

    def _set_relative_levels(self, blocks):
        """One dense pass over the run's first block; its records are dropped and the levels replaced."""
        env = _engine.PinnedBuffer((self.full,), np.int64)
        try:
            self.det.blocks_dev(blocks, 1, self.full, env=env.array)
            self.det.synchronize()
            self.floor = float(np.median(env.array)) / self.spec["W"]
        finally:
            env.close()
        self.det.clear_events()
        base = self.floor / _pulse.POWER_UNIT
        self.det.set_params(base * 10.0 ** (self.spec["on_db"] / 10.0), base * 10.0 ** (self.spec["off_db"] / 10.0))

    def feed_raw(self, blocks, got):
        """blocks: the batch buffer, whose first `got` rows are the run's next blocks."""
        if self.spec["rel"] and self.floor is None:
            self._set_relative_levels(blocks)
        if self.stream:                              # the first `got` rows of the batch buffer are contiguous
            self.det.process_dev(blocks, got * self.full)
        else:
            self.det.blocks_dev(blocks, got, self.full)
        _gather_events(self, self.det, got)

    def handoff(self, d):
        """The hand-off arrays, the INFO line, pulsesSave.  The stream form first closes the pulse still open at the end."""
        if self.stream:
            self.det.flush()
            _gather_events(self, self.det, 0)
        _, total, active = self.det.events()
        ev = np.concatenate(self.parts) if self.parts else np.zeros(0, dtype=_pulse.EVENT_DTYPE)
        d["pulseEvents"], d["pulseTotal"], d["pulseActive"] = ev, total, active
        thr_on, thr_off = self.det.thresholds()
        print("INFO:zero_span: pulses blocks [{}], W [{}], thr_on [{}] thr_off [{}], pulses stored [{}] / total [{}], active samples [{}]".format(
            self.blocks_done, self.det.W, thr_on, thr_off, len(ev), total, active))
        if d["pulsesSave"]:
            s = self.spec
            with open(d["pulsesSave"], "wb") as f:
                np.savez(f, events=ev, pulses_total=np.int64(total), active_total=np.int64(active), rel=np.bool_(s["rel"]),
                         on_db=np.float64(s["on_db"]), off_db=np.float64(s["off_db"]), W=np.int32(s["W"]),
                         min_len=np.int32(s["min_len"]), capacity=np.int32(s["capacity"]), thr_on=np.int64(thr_on),
                         thr_off=np.int64(thr_off), sampling_rate=np.float64(self.rate), block_len=np.int64(self.full),
                         **({"continuous": np.bool_(True)} if self.stream else {}),
                         **_pulse.describe(ev, s["W"], self.rate, 0 if self.stream else self.full))

    def close(self):
        self.det.close()


class _IqFeed:
    """The iqfix key's state over a run: the IqCorrector in front of everything else.  It reads every batch's raw blocks in
    their iqFormat from the page-locked batch buffer and leaves [got][block_len] complex64 in its own buffer.  Without track
    the first batch's first `blocks` blocks are measured and solved once, before anything runs; with track every batch is
    measured in the pass that corrects it, and what it solves to corrects the next one."""

    def __init__(self, d, spec, run):
        self.spec, self.full = spec, run.block_len       # zoom's block length or fullSize: it never runs with channels
        self.fix = IqCorrector(fmt=run.fmt, max_in=run.batch * run.block_len, device=d["device"])
        self.batches, self.solves = 0, []

    @property
    def out_ptr(self):
        return self.fix.out_ptr

    def _solve(self):
        sums = self.fix.read_stats()
        sol = self.fix.solve(self.spec["mode"])
        self.solves.append((self.batches, sol, sums))

    def feed_raw(self, blocks, got):
        """blocks: the batch buffer, whose first `got` rows are the run's next blocks; out_ptr is where their corrected form lies."""
        if self.spec["track"]:
            self.fix.blocks_dev(blocks, got, self.full, accumulate=True)
            self._solve()                            # synchronises; the new coefficients serve the next batch
            self.fix.clear_stats()
        else:
            if not self.solves:
                self.fix.accumulate_dev(blocks, min(self.spec["blocks"] or got, got), self.full)
                self._solve()
            self.fix.blocks_dev(blocks, got, self.full)
        self.batches += 1

    def handoff(self, d):
        """The hand-off dict, the INFO line, iqfixSave."""
        sol = [s for _, s, _ in self.solves]
        derived = [_iqfix.imbalance_of(s["c"], s["d"]) for s in sol]
        out = {"batch": np.array([b for b, _, _ in self.solves], dtype=np.int64),
               "sums": np.array([m for _, _, m in self.solves], dtype=np.int64).reshape(-1, 6),
               "flags": np.array([s["flags"] for s in sol], dtype=np.int32),
               "count": np.array([s["count"] for s in sol], dtype=np.int64),
               "gain_db": np.array([g for g, _ in derived], dtype=np.float64),
               "phase_deg": np.array([p for _, p in derived], dtype=np.float64)}
        for k in ("dc_i", "dc_q", "c", "d"):
            out[k] = np.array([s[k] for s in sol], dtype=np.float32)
        d["iqfix"] = out
        last = sol[-1] if sol else self.fix.get_coeffs()
        print("INFO:zero_span: iqfix batches [{}], solves [{}], last dc [{}] [{}] c [{}] d [{}] flags [{}]".format(
            self.batches, len(sol), last["dc_i"], last["dc_q"], last["c"], last["d"], last["flags"]))
        if d["iqfixSave"]:
            with open(d["iqfixSave"], "wb") as f:
                np.savez(f, mode=np.int32(self.spec["mode"]), track=np.bool_(self.spec["track"]),
                         blocks=np.int64(self.spec["blocks"] or 0), block_len=np.int64(self.full), **out)

    def close(self):
        self.fix.close()


class _DemodFeed:
    """The demod key's state over a run: the Demodulator behind the down-converter, fed every batch's zoomed blocks in device
    memory; each block is demodulated on its own and the blocks abut in the audio.  Under continuous the blocks are one stream:
    detector, filter history and the resampler's position are carried on the device from batch to batch."""

    def __init__(self, d, spec, run):
        self.spec, self.full, batch = spec, d["fullSize"], run.batch
        self.stream = bool(d.get("continuous"))
        fs = d["samplingRate"] / run.front["decim"]
        taps = demod_taps(spec["decim"], spec["taps_per_phase"], deemph_us=spec["deemph_us"],
                          sampling_rate=fs if spec["deemph_us"] is not None else None, dc_block=spec["mode"] == "am")
        self.rspec, self.res = d.get("resample.spec"), None
        self.rate = spec["rate"] if self.rspec is None else self.rspec["rate"]
        self.per_block = spec["out_per_block"] if self.rspec is None else self.rspec["out_per_block"]
        self.dem = Demodulator(spec["mode"], spec["decim"], taps, out_fmt="s16" if self.rspec is None else "f32",
                               pcm_scale=DEMOD_PCM_SCALE, max_in=batch * self.full, device=d["device"])
        if self.rspec is not None:                   # audioRate: float32 audio goes on to the resampler, which makes the int16
            r = self.rspec                           # continuous: in_per_block is the most of a block, one more for the call's rounding
            self.res = Resampler(r["L"], r["M"], resample_taps(r["L"], r["M"], r["taps_per_phase"]), type="f32", out_fmt="s16",
                                 pcm_scale=DEMOD_PCM_SCALE, max_in=batch * r["in_per_block"] + self.stream, device=d["device"])
        self.parts = []

    def _feed_stream(self, iq_dev, got):
        """The batch as the next got x fullSize samples of one stream (kdm_process_dev, then krs_process_dev): a call yields
        ceil(N1 / D) - ceil(N0 / D) values, and the audio of the batches joins with no gap and no repeat."""
        m = self.dem.process_dev(iq_dev, got * self.full)
        if self.res is None:
            self.parts.append(self.dem.read_out(m))
            return
        j = self.res.process_dev(self.dem._out, m)         # both on the NULL stream: the demodulator's values come first
        self.parts.append(self.res.read_out(j))

    def feed(self, iq_dev, got, stride=None):
        """iq_dev: [got][fullSize] complex64 in device memory, the down-converter's own buffer (or, with a stride in values,
        one channel of every block of the channelizer's)."""
        if self.stream:
            assert stride is None                        # both front ends leave a continuous run's frames back to back
            return self._feed_stream(iq_dev, got)
        m = self.dem.blocks_dev(iq_dev, got, self.full, block_stride=stride)
        if self.res is None:
            self.parts.append(self.dem.read_out(got * m))
            return
        j = self.res.blocks_dev(self.dem._out, got, m)     # both on the NULL stream: the demodulator's blocks come first
        self.parts.append(self.res.read_out(got * j))

    def handoff(self, d):
        """The hand-off array, the INFO line, demodSave."""
        pcm = np.concatenate(self.parts) if self.parts else np.zeros(0, dtype=np.int16)
        d["demodAudio"], d["demodRate"] = pcm, self.rate
        print("INFO:zero_span: demod [{}]: [{}] samples at [{}] Hz, {}, peak [{}]".format(
            self.spec["mode"], len(pcm), self.rate, "continuous" if self.stream else "[{}] per block".format(self.per_block),
            int(np.abs(pcm.astype(np.int32)).max()) if len(pcm) else 0))
        if d["demodSave"]:
            write_wav(d["demodSave"], pcm, self.rate)

    def close(self):
        self.dem.close()
        if self.res is not None:
            self.res.close()


class _ZoomFeed:
    """The zoom key's state over a run: the DownConverter in front of the engine, fed every batch's raw blocks -- or, behind
    iqfix, the corrector's complex64 ones; its [got][fullSize] complex64 outputs go on from its own buffer.  Under continuous the
    batch is the next got x block_len samples of one stream (kdc_process_dev): mixer phase and filter history carry on."""

    def __init__(self, d, spec, run):
        self.block_len, self.full, self.stream = spec["block_len"], d["fullSize"], bool(d.get("continuous"))
        fmt = FMT_C64 if d.get("iqfix.spec") is not None else run.fmt
        self.ddc = DownConverter(fmt, spec["decim"], ddc_lowpass(spec["decim"], spec["taps_per_phase"]), freq=spec["offset"],
                                 sampling_rate=d["samplingRate"], max_in=run.batch * self.block_len, device=d["device"])

    def front(self, src, got):
        """(address, no stride) of [got][fullSize] complex64; src is the batch buffer or the corrector's address."""
        if self.stream:                              # block_len = decim x fullSize: every block yields exactly fullSize values
            n = self.ddc.process_dev(src, got * self.block_len)
            assert n == got * self.full, (n, got, self.full)
        else:
            self.ddc.blocks_dev(src, got, self.block_len)
        return self.ddc.out_ptr, None

    def handoff(self, d):
        """Nothing of its own: the zoomed span is what the engine and the other stages hand off."""

    def close(self):
        self.ddc.close()


class _ChanFeed:
    """The channels key's state over a run: the Channelizer in front of the engine, fed every batch's raw blocks; the picked
    channel of every block goes on as a strided view of its buffer, and every channel's power is summed over the run.  Under
    continuous the batch is the next got x block_len samples of one stream (kch_process_dev): the picked channel is one row of
    the bank's buffer, got x fullSize columns back to back."""

    def __init__(self, d, spec, run):
        self.spec, self.full, self.stream = spec, d["fullSize"], bool(d.get("continuous"))
        self.bank = Channelizer(run.fmt, spec["nchan"], spec["oversample"], chan_prototype(spec["nchan"], spec["taps_per_branch"]),
                                max_in=run.batch * spec["block_len"], device=d["device"])
        self.power, self.values = np.zeros(spec["nchan"], dtype=np.float64), 0

    def front(self, blocks, got):
        """(address, stride in values) of the picked channel of every block: [got][M][fullSize] complex64 in the bank's buffer."""
        if self.stream:
            cols = self.bank.process_dev(blocks, got * self.spec["block_len"])
            assert cols == got * self.full, (cols, got, self.full)
            self.power += self.bank.channel_power(0, cols)
            self.values += cols
            return self.bank.out_ptr + 8 * self.spec["pick"] * self.bank.layout()[1], None
        cols = self.bank.blocks_dev(blocks, got, self.spec["block_len"])
        assert cols == self.full
        self.power += self.bank.channel_power(0, cols)
        self.values += got * cols
        return self.bank.out_ptr + 8 * self.spec["pick"] * cols, self.spec["nchan"] * cols

    def handoff(self, d):
        """The hand-off arrays, the INFO line, channelsSave."""
        s = self.spec
        with np.errstate(divide="ignore"):
            db = 10 * np.log10(self.power / max(self.values, 1))
        freqs = channel_freqs(s["nchan"], d["samplingRate"], d["centerFreq"])
        d["channelsPower"], d["channelsFreqs"] = db, freqs
        top = np.argsort(-db, kind="stable")[:3]
        print("INFO:zero_span: channels [{}]: [{}] values per channel, strongest {}".format(
            s["nchan"], self.values, ", ".join("[{}] at [{}] Hz [{:.2f}] dB".format(int(c), freqs[c], db[c]) for c in top)))
        if d["channelsSave"]:
            with open(d["channelsSave"], "wb") as f:
                np.savez(f, power_db=db, freqs=freqs, nchan=s["nchan"], oversample=s["oversample"],
                         taps_per_branch=s["taps_per_branch"], pick=s["pick"], values=self.values,
                         sampling_rate=d["samplingRate"], center_freq=d["centerFreq"])

    def close(self):
        self.bank.close()


def _zero_span_frames(d, eng, freqs):
    """frameBatch 1: the reference's loop, one block per pass."""
    prev = time.time()
    for i in range(d["prgLoopCnt"]):
        now = time.time()
        print("ZeroSpan:{}:{}".format(i, now - prev))
        prev = now
        eng.set_flags(d["bDataMax"], d["bDataMin"], d["bDataAvg"])          # GUI toggles K:471-476
        if sdr_curscan is _gpu_curscan and not d["bUsePSD"]:
            try:
                eng.frame(sdr_read(d["sdr"], d["fullSize"], raw=raw_format(d)))   # fused K:464-484
            except EOFError:
                prg_quit(d, "WARN:zero_span: source exhausted, stoping...", False)
        else:
            try:
                cur = sdr_curscan(d)                                        # rebound seam (playback, K:543) / bUsePSD
            except EOFError:
                cur = None
                prg_quit(d, "WARN:zero_span: source exhausted, stoping...", False)
            if cur is not None:
                eng.frame_spectrum(cur)
        if d["cmd.stop"]:
            break
        _handoff(d, eng, freqs)                  # xRes-sized curves + markers + the new waterfall row (row f2)


def _frames_one_by_one(eng, src, got, full_size, db):
    """A continuous run's batch into the engine one frame per call.  The engine folds the average of a call in closed form
    (ksa.h at ksa_frames_dev), whose float32 rounding depends on the frames per call; the reference's recursion (a + x) / 2 per
    frame, which is what frameBatch 1 computes, does not.  A continuous run promises that nothing it hands off depends on how
    it was cut into batches, so its Fft.Avg is the recursion's at every frameBatch; Cur, Max, Min and the waterfall are the same
    either way.  src: a device address of [got][full_size] complex64 with db = the batch's [got][fftSize] row buffer or None --
    or the page-locked batch itself (full_size None) with db = whether rows are wanted; the dB rows are returned, or None."""
    if full_size is not None:
        for i in range(got):
            eng.frames_dev(src + 8 * i * full_size, FMT_C64, 1, cur_db=None if db is None else db[i:i + 1])
        return db
    out = [eng.frames(src[i:i + 1], cur_db=True)[0] if db else eng.frames(src[i:i + 1]) for i in range(got)]
    return np.concatenate(out) if db else None


def _zero_span_batches(d, eng, run, stages):
    """The batch route: up to run.batch blocks are read into ONE page-locked buffer and go through the engine and the stages in
    one pass; flags, the progress line and the plot refresh come once per batch.  prgLoopCnt still counts frames, and a source
    that runs out mid-batch stops the run after the whole blocks it delivered: the frames are those of frameBatch 1.  Per batch,
    in this order:
    - the corrector (feed_raw + out_ptr: iqfix) reads the raw batch and leaves [got][block_len] complex64 in its own buffer,
      which stands in for the batch from here to the engine;
    - a front end (front: zoom | channels) reads that and returns (address, stride) of [got][fullSize] complex64 on the device;
    - the engine takes those blocks from device memory (ksa_frames_dev), else the batch itself (ksa_frames_c64 / _u8; int8 /
      int16 blocks are read by the kernels from the page-locked buffer), and returns the batch's dB rows if a row stage is on;
    - the demodulator (feed: demod, audioRate) reads the front end's blocks and keeps the batch's int16 audio on the host;
    - the row stages (feed_rows: density, mask, detect) read the dB rows; counts and events stay on the GPU until the hand-off;
    - the raw stages (feed_raw: correlate, pulses) read the page-locked batch and keep the new events, block counted over the run.
    Under continuous the order is the same; the blocks come from one sources.ContiguousReader, which wastes no sample between
    them, every stage that has a stream form takes the batch as the next piece of one stream (what it hands on has the same
    shape), and the engine takes the batch one frame per call (_frames_one_by_one), so that Fft.Avg does not depend on frameBatch."""
    fix = next((s for s in stages if hasattr(s, "feed_raw") and hasattr(s, "out_ptr")), None)
    front = next((s for s in stages if hasattr(s, "front")), None)
    audio = next((s for s in stages if hasattr(s, "feed")), None)
    rows = [s for s in stages if hasattr(s, "feed_rows")]
    raws = [s for s in stages if hasattr(s, "feed_raw") and s is not fix]
    u8, full = run.raw, run.block_len                                        # what sdr_read(..., raw) delivers
    dtype, per = raw_dtype(u8)
    stage = _engine.PinnedBuffer((run.batch, per * full), dtype)
    blocks = stage.array
    read_blocks = getattr(d["sdr"], "read_blocks", None)
    if d.get("continuous"):                      # back to back: block i is samples [i, i + 1) x block_len after the settle read
        read_blocks = sources.ContiguousReader(d["sdr"]).read_blocks
    try:
        done, prev = 0, time.time()
        while done < d["prgLoopCnt"]:
            k = min(run.batch, d["prgLoopCnt"] - done)
            now = time.time()
            print("ZeroSpan:{}:{}".format(done, now - prev))
            prev = now
            eng.set_flags(d["bDataMax"], d["bDataMin"], d["bDataAvg"])      # GUI toggles K:471-476, once per batch
            if read_blocks is not None:
                got = read_blocks(k, full, u8, blocks)
            else:
                got = 0
                try:
                    while got < k:
                        blocks[got] = sdr_read(d["sdr"], full, raw=u8)
                        got += 1
                except EOFError:
                    pass
            if got:
                src, stride, db = blocks, None, None
                if fix is not None:
                    fix.feed_raw(blocks, got)
                    src = fix.out_ptr
                if front is not None:
                    src, stride = front.front(src, got)
                if src is not blocks:                                        # [got][fullSize] complex64 in device memory
                    if rows:
                        db = eng._pinned_out("db", (got, d["fftSize"]))
                    if d.get("continuous"):                                  # frame by frame, see _frames_one_by_one
                        _frames_one_by_one(eng, src, got, d["fullSize"], db)
                    else:
                        eng.frames_dev(src, FMT_C64, got, cur_db=db, frame_stride=stride)
                    eng.synchronize()
                    if audio is not None:
                        audio.feed(src, got, stride)
                elif d.get("continuous"):
                    db = _frames_one_by_one(eng, blocks, got, None, bool(rows))
                elif rows:
                    db = eng.frames(blocks[:got], cur_db=True)[0]
                else:
                    eng.frames(blocks[:got])                                 # K:464-484 for the whole batch, one call
                for s in rows:
                    s.feed_rows(db)
                for s in raws:
                    s.feed_raw(blocks, got)
            done += got
            if got < k:
                prg_quit(d, "WARN:zero_span: source exhausted, stoping...", False)
            if d["cmd.stop"]:
                break
            _handoff(d, eng, run.freqs, new_rows=min(got, _engine.HM_ROWS))  # once per batch: the batch's newest rows
    finally:
        stage.close()


# spec key -> stage class, in the order of construction and of the hand-off; the row stages and the raw stages are fed in it
_STAGES = (("density.spec", _DensityFeed), ("mask.spec", _MaskFeed), ("detect.spec", _DetectFeed), ("demod.spec", _DemodFeed),
           ("zoom.spec", _ZoomFeed), ("chan.spec", _ChanFeed), ("corr.spec", _CorrFeed), ("pulse.spec", _PulseFeed),
           ("iqfix.spec", _IqFeed))


def zero_span_save(d):
    """K:510-526: header then (time, linear spectrum) records; same stream the reference writes."""
    with open(d["zeroSpanSaveFile"], "wb+") as f:
        for k in ("centerFreq", "samplingRate", "gain"):
            pickle.dump(d[k], f)
        d["sdr"], _ = sdr_setup(d["sdr"], d["centerFreq"], d["samplingRate"], d["gain"])
        prev = time.time()
        for i in range(d["prgLoopCnt"]):
            if d["cmd.stop"]:
                break
            now = time.time()
            print("ZeroSpanSave:{}:{}".format(i, now - prev))
            prev = now
            try:
                cur = sdr_curscan(d)
            except EOFError:
                break
            pickle.dump(now, f)
            pickle.dump(cur, f)


def zero_span_play_setup(d):
    """K:530-543: the file's header overrides centre / rate / gain and `sdr_curscan` is rebound."""
    global sdr_curscan
    d["zeroSpanFile"] = f = open(d["zeroSpanPlayFile"], "rb")
    d["centerFreq"], d["samplingRate"], d["gain"] = _load(f), _load(f), _load(f)
    d["startFreq"], d["endFreq"] = _calc_startendfreq(d["centerFreq"], d["samplingRate"])
    sdr_curscan = zero_span_play


def zero_span_play(d):
    """K:547-564: next saved spectrum, or None (and cmd.stop) at the end of the file."""
    try:
        d["timeWas"] = _load(d["zeroSpanFile"])
        ms = int((d["timeWas"] - int(d["timeWas"])) * 1000)
        d["timeWasStr"] = "{}.{:03}".format(time.strftime("%Y%m%d%Z%H%M%S", time.gmtime(d["timeWas"])), ms)
        print("INFO:zeroSpanPlay:timeWas:{}".format(d["timeWasStr"]))
        return _load(d["zeroSpanFile"])
    except Exception:
        prg_quit(d, "WARN:zero_span_play:loading failed, stoping...", False)
        return None


# ------------------------------------------------------------------------------------------------ scan
def scan_geometry(d):
    """K:587-600, K:621, K:689-690: (numGroups, totalEntries, tuned centre of every step)."""
    span = d["samplingRate"]
    q = d["scanRangeNonOverlap"]
    if ((span * q) % 1) != 0:
        prg_quit(d, "ERROR: freqSpan [{}] x scanRangeNonOverlap [{}] is not int".format(span, q))
    if ((d["fftSize"] * q) % 1) != 0:
        prg_quit(d, "ERROR: fftSize[{}] x scanRangeNonOverlap [{}] is not int".format(d["fftSize"], q))
    groups = int((d["endFreq"] - d["startFreq"]) / span)
    centers, cur = [], d["startFreq"] + span / 2
    while cur - span / 2 < d["endFreq"]:
        centers.append(cur)
        cur += span * q
    return groups, groups * d["fftSize"], centers


def scan_range(d):
    """K:712-732 with _scan_range (K:568-698): per pass, capture every tuned band, then one device call
    stitches the bands and updates Cur/Max/Min/Avg and the waterfall row."""
    _fixupfreqs_scanrange(d)
    groups, total, centers = scan_geometry(d)
    print("_scanRange: start:{} end:{} samplingRate:{}".format(d["startFreq"], d["endFreq"], d["samplingRate"]))
    print("_scanRange: totalFreqs:{} numGroups:{} totalEntries:{}".format(d["endFreq"] - d["startFreq"], groups, total))
    steps = len(centers)
    if d["bUsePSD"]:
        print("WARN:_scanRange: bUsePSD is a zeroSpan diagnostic here (the whole pass is one device call); ignored")
    eng = get_engine(d, scan_total=total, max_frames=steps)
    eng.scan_reset()
    eng.scan_set_base_is_raw(d["bScanRangeBaseDataIsRaw"])
    span = groups * d["samplingRate"]
    d["freqsAll"] = np.fft.fftshift(np.fft.fftfreq(total, 1 / span) + d["startFreq"] + span / 2)   # K:609
    u8 = raw_format(d)
    # one pass of capture blocks in page-locked host memory; the library stages it to the GPU (ksa_scan_pass_c64 / _u8), or the
    # kernels read it from there (int8 / int16 I,Q: ksa_scan_pass_dev)
    dtype, per = raw_dtype(u8)
    stage = _engine.PinnedBuffer((steps, per * d["fullSize"]), dtype)
    blocks = stage.array
    d["fftHM"], d["fftHMIndex"] = eng.hm_rows(0, _engine.HM_ROWS, scan=True), 0    # K:613-614, read once
    survey, sv = None, d.get("survey.spec")
    if sv is not None:        # scanDetect: the pass goes through the survey, which leaves the engine what eng.scan_pass leaves
        survey = ScanSurvey(eng, steps, sv["train"], sv["guard"], sv["threshold"], mode=sv["mode"], min_width=sv["min_width"],
                            max_gap=sv["max_gap"], capacity=sv["capacity"], edge=sv["edge"], dc=sv["dc"], cells=d["xRes"])
    began = prev = time.time()
    for i in range(d["prgLoopCnt"]):
        if d["cmd.stop"]:
            break
        now = time.time()
        print("scanRange:{}:{}".format(i, now - prev))
        prev = now
        ok = np.ones(steps, dtype=np.uint8)
        for s, fc in enumerate(centers):
            d["sdr"], bOk = sdr_setup(d["sdr"], fc, d["samplingRate"], d["gain"])
            if not bOk:
                print("WARN:_scanRange: Dummy data for {} to {}".format(fc - d["samplingRate"] / 2, fc + d["samplingRate"] / 2))
                ok[s] = 0                                                   # K:637-639
                continue
            blocks[s] = sdr_read(d["sdr"], d["fullSize"], raw=u8)
        eng.set_flags(d["bDataMax"], d["bDataMin"], True)
        if survey is None:
            eng.scan_pass(blocks, step_ok=ok)
        else:
            survey.scan_pass(blocks, step_ok=ok)
        _handoff(d, eng, d["freqsAll"], scan=True)
    _materialize(d, eng, scan=True)
    stage.close()
    if survey is not None:
        try:
            _survey_handoff(d, survey, time.time() - began)
        finally:
            survey.close()


def _survey_handoff(d, survey, elapsed_s):
    """The scanDetect key's hand-off arrays, the INFO line, scanDetectSave; then, with the scanTrack key, the link over the
    passes, its hand-off arrays, INFO line and scanTrackSave.  A row of the tracker is a pass: row_period_s is the measured mean
    time per pass."""
    s, freqs = d["survey.spec"], d["freqsAll"]
    ev, members, total = survey.emissions()
    occ, passes, counters = survey.occupancy(), survey.passes, dict(survey.counters)
    d["surveyEmissions"], d["surveyMembers"], d["surveyEmissionsTotal"] = ev, members, total
    d["surveyCounters"], d["surveyOccupancy"], d["surveyPasses"] = counters, occ, passes
    busiest = int(np.argmax(occ))
    print("INFO:scan_range: survey passes [{}], emissions stored [{}] / total [{}], dropped dc [{}] edge [{}] clipped [{}], "
          "highest occupancy [{:.6f}] at cell [{}] of [{}]".format(
              passes, len(ev), total, counters["dc_dropped"], counters["edge_dropped"], counters["clipped"],
              float(occ[busiest]) / passes if passes else 0.0, busiest, len(occ)))
    if survey.band_lost:
        print("WARN:scan_range: [{}] band emissions exceeded the detector's [{}] per pass and were not stitched".format(
            survey.band_lost, survey.band_capacity))
    if d["scanDetectSave"]:
        center, width = emission_freqs(ev, freqs)
        with open(d["scanDetectSave"], "wb") as f:
            np.savez(f, emissions=ev, members=members, emissions_total=np.int64(total), occupancy=occ, passes=np.int64(passes),
                     train=np.int32(s["train"]), guard=np.int32(s["guard"]), threshold_db=np.float32(s["threshold"]),
                     mode=np.array(s["mode"]), min_width=np.int32(s["min_width"]), max_gap=np.int32(s["max_gap"]),
                     edge=np.int32(s["edge"]), dc=np.int32(s["dc"]), center_hz=center, width_hz=width,
                     peak_hz=np.asarray(freqs, dtype=np.float64)[ev["peak_bin"]],
                     **{k: np.int64(v) for k, v in counters.items()})
    t = d.get("surveyTrack.spec")
    if t is None:
        return
    row_period_s = elapsed_s / passes if passes else 0.0
    tr, tracks_total, comps, labels = survey.link(t["row_gap"], t["bin_slop"], min_rows=t["min_rows"], min_spans=t["min_spans"],
                                                  capacity=t["capacity"])
    d["surveyTracks"], d["surveyTrackTotal"], d["surveyTrackComponents"], d["surveyTrackLabels"] = tr, tracks_total, comps, labels
    longest = int((tr["row_last"] - tr["row_first"] + 1).max()) if len(tr) else 0
    print("INFO:scan_range: survey track emissions [{}], components [{}], tracks stored [{}] / total [{}], longest [{}] passes, "
          "open at the end [{}]".format(len(labels), comps, len(tr), tracks_total, longest,
                                        int(np.count_nonzero(tr["flags"] & _track.FLAG_OPEN_END))))
    if d["scanTrackSave"]:
        with open(d["scanTrackSave"], "wb") as f:
            np.savez(f, tracks=tr, tracks_total=np.int64(tracks_total), components_total=np.int64(comps), labels=labels,
                     row_gap=np.int32(t["row_gap"]), bin_slop=np.int32(t["bin_slop"]), min_rows=np.int32(t["min_rows"]),
                     min_spans=np.int32(t["min_spans"]), capacity=np.int32(t["capacity"]),
                     row_period_s=np.float64(row_period_s), **track_times_freqs(tr, freqs, row_period_s))


# ------------------------------------------------------------------------------------------------ main
def do_run(d):
    """K:1126-1136."""
    if d["prgMode"] == "SCAN":
        scan_range(d)
    elif d["prgMode"] == "ZEROSPANSAVE":
        zero_span_save(d)
    elif d["prgMode"] == "ZEROSPANPLAY":
        zero_span_play_setup(d)
        zero_span(d)
        d["zeroSpanFile"].close()
    else:
        zero_span(d)


gD = None     # the reference's module-level state dict (K:1139); handle_sigint needs it


def handle_sigint(signum, stack):
    """K:1118-1119."""
    prg_quit(gD, "INFO:sigint: quiting on user request...")


def handle_signals(d):
    """K:1122-1123."""
    signal.signal(signal.SIGINT, handle_sigint)


def main(argv=None):
    global sdr_curscan, gD, _reopen_source
    sdr_curscan = _gpu_curscan
    d = gD = {"cmd.stop": False}
    handle_args(d, argv)
    _load_siglvls(d)
    print_info(d)
    handle_signals(d)
    _reopen_source = lambda: open_source(d)
    plt_figures(d)
    d["sdr"] = None if d["prgMode"] == "ZEROSPANPLAY" else open_source(d)   # playback needs no SDR (appendix B)
    if d["sdr"] is not None:
        sdr_info(d["sdr"])                                                   # K:1147
    try:
        do_run(d)
    finally:
        if d.get("sdr") is not None:
            d["sdr"].close()
        if d.get("ksa.engine") is not None:
            d["ksa.engine"].close()
            d["ksa.engine"] = None
    _save_siglvls(d)
    return d


if __name__ == "__main__":
    main()
