"""Digital down-converter (zoom) front end on the GPU: ctypes binding of include/ksa_ddc.h (libksa_ddc.so, a companion of
libksa.so) and the DownConverter class over it.  The frequency of interest is shifted to 0 Hz, low-pass filtered and decimated
by D; the complex64 result in device memory is what the engine's frames_dev / curscan_dev / scan entry points already accept,
and the same fftSize then resolves D times finer bins.  There is no fallback: a missing library raises."""
import ctypes as C
from fractions import Fraction

import numpy as np

from ._companion import Binding, Companion, host_iq
from ._lib import KsaError, FMT_C64, FMT_U8, FMT_S8, FMT_S16
from .engine import DevArray, _ptr, window_table

ABI_VERSION = 1
MAX_DECIM, MAX_TAPS, MAX_IN = 1024, 16384, 2 ** 28 - 1
FORM_TILE, FORM_REDUCE = 0, 1

_P = C.c_void_p
_I32, _I64, _U64, _F = C.c_int32, C.c_int64, C.c_uint64, C.c_float

# name -> (restype, argtypes); every symbol include/ksa_ddc.h declares
SIGNATURES = {
    "kdc_abi_version": (C.c_int, []),
    "kdc_last_error": (C.c_char_p, []),
    "kdc_create": (C.c_int, [_I32, _I32, _F, _F, _I32, _I32, _P, _U64, _I64, C.POINTER(_P)]),
    "kdc_destroy": (None, [_P]),
    "kdc_set_stream": (C.c_int, [_P, _P]),
    "kdc_synchronize": (C.c_int, [_P]),
    "kdc_out_count": (C.c_int, [_P, _I64, C.POINTER(_I64)]),
    "kdc_process_dev": (C.c_int, [_P, _P, _I64, _P, _I64, C.POINTER(_I64)]),
    "kdc_process": (C.c_int, [_P, _P, _I64, _P, _I64, C.POINTER(_I64)]),
    "kdc_blocks_dev": (C.c_int, [_P, _P, _I64, _I64, _I64, _P, _I64]),
    "kdc_set_tuning": (C.c_int, [_P, _U64]),
    "kdc_set_taps": (C.c_int, [_P, _P]),
    "kdc_reset": (C.c_int, [_P]),
    "kdc_state": (C.c_int, [_P, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(_U64)]),
    "kdc_out_dev": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_I64)]),
    "kdc_kernel_info": (C.c_int, [_P] + [C.POINTER(_I32)] * 6),
}


_bind = Binding("libksa_ddc.so", "kdc_", ABI_VERSION, SIGNATURES)
LIB_PATH = _bind.path
load, lib, check = _bind.load, _bind.lib, _bind.check


def phase_inc_for(freq, sampling_rate):
    """round(freq / sampling_rate * 2^64) mod 2^64 as an exact integer: the mixer step that brings a signal at +freq to 0 Hz."""
    turns = Fraction(freq) / Fraction(sampling_rate)
    return int(round(turns * 2 ** 64)) % 2 ** 64


def ddc_lowpass(decim, taps_per_phase=8, cutoff=0.8, window="hamming"):
    """float32 [decim * taps_per_phase]: sinc(cutoff * t / decim) * window_table(window, T) with t centred, normalised in
    float64 to sum 1, so that a pass-band tone keeps its amplitude.  cutoff 1.0 puts the -6 dB point at the edge of the
    decimated band, fs / (2 decim)."""
    decim, taps_per_phase = int(decim), int(taps_per_phase)
    n = decim * taps_per_phase
    if not (1 <= decim <= MAX_DECIM and taps_per_phase >= 1 and n <= MAX_TAPS and 0 < cutoff <= 1):
        raise KsaError("ddc_lowpass wants decim 1..%d, decim * taps_per_phase 1..%d and 0 < cutoff <= 1" % (MAX_DECIM, MAX_TAPS))
    t = np.arange(n, dtype=np.float64) - (n - 1) / 2
    h = np.sinc(cutoff * t / decim) * np.asarray(window_table(window, n), dtype=np.float64)
    return (h / h.sum()).astype(np.float32)


class DownConverter(Companion):
    """Mixer, real FIR low-pass and decimator by `decim` for one IQ stream on one GPU; the contract is include/ksa_ddc.h.
    The tuning is either phase_inc (2^64 = one turn per input sample) or freq with sampling_rate."""
    _binding, _info_fields = _bind, ("threads", "lds_bytes", "vgprs", "grid", "tile_out", "form")

    def __init__(self, fmt, decim, taps, freq=0.0, sampling_rate=1.0, phase_inc=None, max_in=1 << 20, device=0, stream=None,
                 u8_offset=127.5, u8_scale=127.5):
        self.fmt, self.decim, self.device, self.max_in = int(fmt), int(decim), int(device), int(max_in)
        self.sampling_rate = sampling_rate
        self.taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        self.ntaps = int(self.taps.size)
        inc = phase_inc_for(freq, sampling_rate) if phase_inc is None else int(phase_inc) % 2 ** 64
        self._create(self.device, self.fmt, u8_offset, u8_scale, self.decim, self.ntaps, _ptr(self.taps), inc, self.max_in,
                     stream=stream)
        self.phase_inc = inc
        p, cap = C.c_void_p(), C.c_int64()
        check(lib().kdc_out_dev(self._h, C.byref(p), C.byref(cap)))
        self._out, self.out_capacity = p.value, cap.value

    # -- the stream form ----------------------------------------------------------------------------
    def out_count(self, n_in):
        n = C.c_int64()
        check(lib().kdc_out_count(self._h, int(n_in), C.byref(n)))
        return n.value

    def process_dev(self, iq, n_in, out=None, out_capacity=0):
        """The stream's next n_in samples from device memory; asynchronous.  out: a device complex64 buffer of out_capacity
        values, or None for the object's own (self.out).  Returns the number of outputs."""
        n = C.c_int64()
        check(lib().kdc_process_dev(self._h, _ptr(iq), int(n_in), _ptr(out), int(out_capacity), C.byref(n)))
        return n.value

    def process(self, samples):
        """The stream's next samples from host memory (complex64 [n], or [2n] uint8 / int8 / int16 I,Q); complex64 outputs;
        synchronises."""
        a, n_in = host_iq(samples, self.fmt)
        out = np.empty(self.out_count(n_in), dtype=np.complex64)
        n = C.c_int64()
        check(lib().kdc_process(self._h, _ptr(a), n_in, _ptr(out), out.size, C.byref(n)))
        return out[:n.value]

    # -- the block form -----------------------------------------------------------------------------
    def block_out_count(self, block_len):
        return (int(block_len) - self.ntaps) // self.decim + 1

    def blocks_dev(self, iq, nblocks, block_len, block_stride=None, out=None, out_stride=None):
        """nblocks independent captures of block_len samples, block b at iq + b*block_stride samples (device memory or
        PinnedBuffer.array); asynchronous.  out None: the object's own buffer at stride M.  Returns M, the outputs per block."""
        m = self.block_out_count(block_len)
        stride = int(block_len) if block_stride is None else int(block_stride)
        check(lib().kdc_blocks_dev(self._h, _ptr(iq), stride, int(nblocks), int(block_len), _ptr(out),
                                   m if out_stride is None else int(out_stride)))
        return m

    # -- state --------------------------------------------------------------------------------------
    def retune(self, freq=None, sampling_rate=None, phase_inc=None):
        """A new tuning from the next input sample on; the phase stays continuous."""
        if phase_inc is None:
            phase_inc = phase_inc_for(freq, self.sampling_rate if sampling_rate is None else sampling_rate)
        check(lib().kdc_set_tuning(self._h, int(phase_inc) % 2 ** 64))
        self.phase_inc = int(phase_inc) % 2 ** 64

    def set_taps(self, taps):
        """Replace the taps (the same count); the history is kept.  Synchronises."""
        t = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        if t.size != self.ntaps:
            raise KsaError("set_taps wants [%d] float32, got %s" % (self.ntaps, t.shape))
        check(lib().kdc_set_taps(self._h, _ptr(t)))
        self.taps = t

    def reset(self):
        check(lib().kdc_reset(self._h))

    def state(self):
        """dict(samples_in, samples_out, phase) of the stream."""
        a, b, p = C.c_int64(), C.c_int64(), C.c_uint64()
        check(lib().kdc_state(self._h, C.byref(a), C.byref(b), C.byref(p)))
        return {"samples_in": a.value, "samples_out": b.value, "phase": p.value}

    @property
    def out(self):
        """The object's output buffer, complex64 [out_capacity], for torch.as_tensor."""
        return DevArray(self._out, (self.out_capacity,), self, "<c8")

    @property
    def out_ptr(self):
        return self._out
