"""Time-domain pulse detector and pulse list on the GPU: ctypes binding of include/ksa_pulse.h (libksa_pulse.so, a companion of
libksa.so) and the PulseDetector class over it.  The power of raw IQ in device memory is summed over W samples, compared with a
trigger level that has hysteresis, and every pulse is listed with its start, width, energy, peak and the sum its carrier offset
is read from.  Every decision and every sum is an integer.  There is no fallback: a missing library raises."""
import ctypes as C

import numpy as np

from ._companion import FORMATS, SAMPLE_DTYPES, Binding, Companion, format_of
from ._lib import KsaError, FMT_C64, FMT_U8, FMT_S8, FMT_S16
from .engine import DevArray, _ptr

ABI_VERSION = 1
MAX_W, MAX_MIN_LEN, MAX_CAPACITY, MAX_IN, MAX_POSITION = 4096, 1 << 20, 1 << 20, 2 ** 28 - 1, 2 ** 52
POWER_UNIT = 1 << 30                    # q, energy and S count full-scale power in units of 2^-30
FLAG_OPEN_END = 1

_P = C.c_void_p
_I32, _I64, _F = C.c_int32, C.c_int64, C.c_float

# the 64 bytes of kpl_pulse, no padding
EVENT_DTYPE = np.dtype([("start", "<i8"), ("len", "<i8"), ("energy", "<i8"), ("peak", "<i8"), ("peak_pos", "<i8"), ("dre", "<i8"),
                        ("dim", "<i8"), ("block", "<i4"), ("flags", "<i4")])
assert EVENT_DTYPE.itemsize == 64
PULSE_DTYPE = EVENT_DTYPE              # the name the package exports it under (mask.py and corr.py have an EVENT_DTYPE of their own)

# name -> (restype, argtypes); every symbol include/ksa_pulse.h declares
SIGNATURES = {
    "kpl_abi_version": (C.c_int, []),
    "kpl_last_error": (C.c_char_p, []),
    "kpl_create": (C.c_int, [_I32, _I32, _F, _F, _I32, _F, _F, _I32, _I32, _I64, C.POINTER(_P)]),
    "kpl_destroy": (None, [_P]),
    "kpl_set_stream": (C.c_int, [_P, _P]),
    "kpl_synchronize": (C.c_int, [_P]),
    "kpl_process_dev": (C.c_int, [_P, _P, _I64, _P]),
    "kpl_process": (C.c_int, [_P, _P, _I64, _P]),
    "kpl_flush": (C.c_int, [_P]),
    "kpl_blocks_dev": (C.c_int, [_P, _P, _I64, _I64, _I64, _P, _I64]),
    "kpl_set_params": (C.c_int, [_P, _F, _F]),
    "kpl_thresholds": (C.c_int, [_P, C.POINTER(_I64), C.POINTER(_I64)]),
    "kpl_reset": (C.c_int, [_P]),
    "kpl_state": (C.c_int, [_P, C.POINTER(_I64), C.POINTER(_I32), C.POINTER(_I64)]),
    "kpl_read_events": (C.c_int, [_P, _P, _I64, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(_I64)]),
    "kpl_events_dev": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P)]),
    "kpl_clear_events": (C.c_int, [_P]),
    "kpl_kernel_info": (C.c_int, [_P] + [C.POINTER(_I32)] * 5),
}


_bind = Binding("libksa_pulse.so", "kpl_", ABI_VERSION, SIGNATURES)
LIB_PATH = _bind.path
load, lib, check = _bind.load, _bind.lib, _bind.check


def db_to_power(db):
    """A level in dB relative to full scale (10 log10 of the mean power) as the float32 linear mean power the library takes."""
    return float(np.float32(10.0 ** (float(db) / 10.0)))


class PulseDetector(Companion):
    """A pulse detector on one GPU; the contract is include/ksa_pulse.h.  W: samples of the envelope's sliding sum; on_power and
    off_power: linear mean powers, 0 < off_power <= on_power <= 4.  fmt: c64 | u8 | s8 | s16 (or the number).  It holds the
    first `capacity` pulses in ascending (block, start) order."""
    _binding, _info_fields = _bind, ("threads", "lds_bytes", "vgprs", "grid", "tile")

    def __init__(self, W=16, on_power=0.1, off_power=None, min_len=1, capacity=1024, max_in=1 << 20, fmt="c64", u8_offset=127.5,
                 u8_scale=127.5, device=0, stream=None):
        self.fmt = format_of(fmt)
        self.W, self.min_len = int(W), int(min_len)
        self.on_power = float(on_power)
        self.off_power = self.on_power if off_power is None else float(off_power)
        self.capacity, self.max_in, self.device = int(capacity), int(max_in), int(device)
        self.in_dtype = SAMPLE_DTYPES.get(self.fmt, np.dtype(np.complex64))
        self._create(self.device, self.fmt, float(u8_offset), float(u8_scale), self.W, self.on_power, self.off_power,
                     self.min_len, self.capacity, self.max_in, stream=stream)

    # -- the stream form ----------------------------------------------------------------------------
    def process_dev(self, iq, n_in, env=None):
        """The stream's next n_in samples from device memory; asynchronous.  env: device int64 [n_in] for S, or None."""
        check(lib().kpl_process_dev(self._h, _ptr(iq), int(n_in), _ptr(env)))

    def process(self, samples):
        """The stream's next samples from host memory (complex64 [n], or [n][2] of the integer formats); synchronises.
        Returns S, int64 [n]."""
        a = np.ascontiguousarray(samples, dtype=self.in_dtype)
        n_in = a.size if self.fmt == FMT_C64 else a.size // 2
        env = np.zeros(n_in, dtype=np.int64)
        check(lib().kpl_process(self._h, _ptr(a), n_in, _ptr(env)))
        return env

    def flush(self):
        """Close the run still open at the end of the stream; stream calls are refused afterwards until reset()."""
        check(lib().kpl_flush(self._h))

    # -- the block form -----------------------------------------------------------------------------
    def blocks_dev(self, iq, nblocks, block_len, block_stride=None, env=None, out_stride=None):
        """nblocks independent blocks of block_len samples, block b at iq + b*block_stride samples (device memory);
        asynchronous.  env: device int64, S of block b at b * out_stride; or None."""
        stride = int(block_len) if block_stride is None else int(block_stride)
        check(lib().kpl_blocks_dev(self._h, _ptr(iq), stride, int(nblocks), int(block_len), _ptr(env),
                                   int(block_len) if out_stride is None else int(out_stride)))

    # -- state --------------------------------------------------------------------------------------
    def set_params(self, on_power=None, off_power=None):
        """Replace on_power and off_power (None keeps a value); they hold from the next call."""
        on = self.on_power if on_power is None else float(on_power)
        off = self.off_power if off_power is None else float(off_power)
        check(lib().kpl_set_params(self._h, on, off))
        self.on_power, self.off_power = on, off

    def thresholds(self):
        """(thr_on, thr_off): the integer levels S is compared with."""
        a, b = C.c_int64(), C.c_int64()
        check(lib().kpl_thresholds(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def reset(self):
        check(lib().kpl_reset(self._h))

    def state(self):
        """dict(samples_in, open, open_start) of the stream; open_start is -1 when no run is open.  Synchronises."""
        a, b, c = C.c_int64(), C.c_int32(), C.c_int64()
        check(lib().kpl_state(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"samples_in": a.value, "open": bool(b.value), "open_start": c.value}

    # -- results ------------------------------------------------------------------------------------
    def events(self):
        """(structured array of EVENT_DTYPE: the stored records in ascending (block, start) order; pulses_total;
        active_total); synchronises."""
        stored, total, active = C.c_int64(), C.c_int64(), C.c_int64()
        check(lib().kpl_read_events(self._h, None, 0, C.byref(stored), C.byref(total), C.byref(active)))
        out = np.zeros(stored.value, dtype=EVENT_DTYPE)
        if stored.value:
            check(lib().kpl_read_events(self._h, _ptr(out), stored.value, C.byref(stored), C.byref(total), C.byref(active)))
        return out[:stored.value].copy(), total.value, active.value

    def clear_events(self):
        check(lib().kpl_clear_events(self._h))

    def events_view(self):
        """The record buffer as raw bytes [capacity][64] in device memory, for torch.as_tensor."""
        p = C.c_void_p()
        check(lib().kpl_events_dev(self._h, C.byref(p), None))
        return DevArray(p.value, (self.capacity, EVENT_DTYPE.itemsize), self, "|u1")


def describe(events, W, sampling_rate, full_size=0):
    """What a pulse list says in units: dict of float64 arrays toa_s = (block * full_size + start) / sampling_rate (the stream
    form's block -1 counts as 0), width_s, mean_dbfs = 10 log10(energy / 2^30 / len), peak_dbfs = 10 log10(peak / 2^30 / W) and
    freq_hz = atan2(dim, dre) / 2 pi * sampling_rate."""
    ev = np.asarray(events)
    fs = float(sampling_rate)
    block = np.maximum(ev["block"].astype(np.float64), 0.0)
    ln = np.maximum(ev["len"].astype(np.float64), 1.0)
    with np.errstate(divide="ignore"):
        mean = 10 * np.log10(ev["energy"].astype(np.float64) / POWER_UNIT / ln)
        peak = 10 * np.log10(ev["peak"].astype(np.float64) / POWER_UNIT / float(W))
    return {"toa_s": (block * float(full_size) + ev["start"].astype(np.float64)) / fs,
            "width_s": ev["len"].astype(np.float64) / fs,
            "mean_dbfs": mean, "peak_dbfs": peak,
            "freq_hz": np.arctan2(ev["dim"].astype(np.float64), ev["dre"].astype(np.float64)) / (2 * np.pi) * fs}
