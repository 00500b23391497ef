"""MI355X-native overlapped windowed-FFT spectrum / waterfall engine (kspecanal-compatible).

Python host -> ctypes -> libksa.so (hand-written HIP for gfx950).  Importing this package loads
the library and raises if it is missing: there is no CPU path in the product.  SpectrumDensity (density.py) is the density
(persistence) histogram over the engine's dB rows, in the companion library libksa_density.so; SpectrumMask (mask.py) is the
frequency-mask trigger and per-bin occupancy counter over the same rows, in libksa_mask.so; DownConverter (ddc.py) is the
digital down-converter (zoom) in front of the engine: mixer, low-pass and decimator, in libksa_ddc.so; SignalDetector
(detect.py) is the CFAR signal detector and emission list over the engine's dB rows, in libksa_detect.so; Demodulator
(demod.py) is the AM / FM / PM demodulator behind the zoom: detector, low-pass and decimator, in libksa_demod.so; Channelizer
(chan.py) is the polyphase channelizer between the two: all M channels of a band at once, in libksa_chan.so; Resampler
(resamp.py) is the rational L / M resampler behind any of them: real or complex samples at L / M times the rate, in
libksa_resamp.so; Correlator (corr.py) is the matched-filter correlator and peak list over the raw samples: where in time a
known waveform lies, in libksa_corr.so; PulseDetector (pulse.py) is the time-domain pulse detector and pulse list over the raw
samples: when something was on the air, in libksa_pulse.so; EmissionTracker (track.py) is the linker behind the signal
detector: its per-row emissions joined into time-frequency tracks, a signal list, in libksa_track.so; IqCorrector (iqfix.py)
is the blind DC-offset and IQ-imbalance corrector in front of all of them: raw samples in, corrected complex64 out, and the
integer sums the correction is solved from, in libksa_iqfix.so; ScanSurvey (survey.py) is the detector and the linker under a
scan: the emissions of every tuned band joined over the stitched range, one list per pass, over those same libraries;
SpectrumMeter (measure.py) is the band meter beside the signal detector: channel power, occupied bandwidth, x-dB width, peak
and power centroid of every emission or of fixed channels, in libksa_measure.so.
"""
from ._lib import KsaError, lib, LIB_PATH, FMT_C64, FMT_U8, FMT_S8, FMT_S16, OUT_LINEAR, OUT_DB, OUT_DB_CLIP, HM_ROWS, CUMU_PFB, CUMU_PFB_PSD
from .engine import (SpectrumEngine, PinnedBuffer, allreduce_state, scan_allstitch, scan_gather_state, full_size_for,
                     window_starts, window_table, heatmap_width, fft_size_supported, psd_window_starts, psd_mag_scale,
                     pfb_window)
from .density import SpectrumDensity
from .mask import SpectrumMask, learn_mask
from .ddc import DownConverter, ddc_lowpass, phase_inc_for
from .detect import SignalDetector, EMISSION_DTYPE, emission_freqs
from .demod import Demodulator, demod_taps, write_wav
from .chan import Channelizer, chan_prototype, channel_freqs
from .resamp import Resampler, resample_taps, rate_ratio
from .corr import Correlator, frequency_bank, refine
from .pulse import PulseDetector, PULSE_DTYPE, FLAG_OPEN_END, POWER_UNIT
from .track import EmissionTracker, TRACK_DTYPE, SPAN_DTYPE, track_times_freqs      # track.FLAG_OPEN_END is the same bit 0
from .iqfix import IqCorrector, imbalance_of
from .survey import ScanSurvey, stitch_emissions
from .measure import SpectrumMeter, RESULT_DTYPE, result_freqs, acpr

__all__ = ["KsaError", "SpectrumEngine", "lib", "LIB_PATH", "FMT_C64", "FMT_U8", "FMT_S8", "FMT_S16", "OUT_LINEAR", "OUT_DB",
           "OUT_DB_CLIP", "HM_ROWS", "PinnedBuffer", "allreduce_state", "scan_allstitch", "scan_gather_state", "full_size_for", "window_starts", "window_table", "heatmap_width",
           "fft_size_supported", "psd_window_starts", "psd_mag_scale", "pfb_window", "CUMU_PFB", "CUMU_PFB_PSD", "SpectrumDensity",
           "SpectrumMask", "learn_mask", "DownConverter", "ddc_lowpass", "phase_inc_for",
           "SignalDetector", "EMISSION_DTYPE", "emission_freqs", "Demodulator", "demod_taps", "write_wav",
           "Channelizer", "chan_prototype", "channel_freqs", "Resampler", "resample_taps", "rate_ratio",
           "Correlator", "frequency_bank", "refine", "PulseDetector", "PULSE_DTYPE", "FLAG_OPEN_END", "POWER_UNIT",
           "EmissionTracker", "TRACK_DTYPE", "SPAN_DTYPE", "track_times_freqs", "IqCorrector", "imbalance_of",
           "ScanSurvey", "stitch_emissions", "SpectrumMeter", "RESULT_DTYPE", "result_freqs", "acpr"]
