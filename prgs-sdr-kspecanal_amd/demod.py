"""AM / FM / PM demodulator behind the zoom on the GPU: ctypes binding of include/ksa_demod.h (libksa_demod.so, a companion of
libksa.so) and the Demodulator class over it.  The complex64 block that the down-converter leaves in device memory (or a raw
complex64 capture) becomes amplitude, frequency or phase versus time, low-pass filtered and decimated by D, as float32 or as
int16 PCM.  There is no fallback: a missing library raises."""
import ctypes as C
import wave

import numpy as np

from ._companion import Binding, Companion
from ._lib import KsaError
from .engine import DevArray, _ptr
from .ddc import ddc_lowpass

ABI_VERSION = 1
MODE_AM, MODE_FM, MODE_PM = 0, 1, 2
MODES = {"am": MODE_AM, "fm": MODE_FM, "pm": MODE_PM}
OUT_F32, OUT_S16 = 0, 1
OUT_FMTS = {"f32": OUT_F32, "s16": OUT_S16}
MAX_DECIM, MAX_TAPS, MAX_IN = 256, 4096, 2 ** 28 - 1

_P = C.c_void_p
_I32, _I64, _F = C.c_int32, C.c_int64, C.c_float

# name -> (restype, argtypes); every symbol include/ksa_demod.h declares
SIGNATURES = {
    "kdm_abi_version": (C.c_int, []),
    "kdm_last_error": (C.c_char_p, []),
    "kdm_create": (C.c_int, [_I32, _I32, _I32, _I32, _P, _I32, _F, _I64, C.POINTER(_P)]),
    "kdm_destroy": (None, [_P]),
    "kdm_set_stream": (C.c_int, [_P, _P]),
    "kdm_synchronize": (C.c_int, [_P]),
    "kdm_out_count": (C.c_int, [_P, _I64, C.POINTER(_I64)]),
    "kdm_process_dev": (C.c_int, [_P, _P, _I64, _P, _I64, C.POINTER(_I64)]),
    "kdm_process": (C.c_int, [_P, _P, _I64, _P, _I64, C.POINTER(_I64)]),
    "kdm_blocks_dev": (C.c_int, [_P, _P, _I64, _I64, _I64, _P, _I64]),
    "kdm_set_taps": (C.c_int, [_P, _P]),
    "kdm_reset": (C.c_int, [_P]),
    "kdm_state": (C.c_int, [_P, C.POINTER(_I64), C.POINTER(_I64)]),
    "kdm_out_dev": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_I64)]),
    "kdm_read_out": (C.c_int, [_P, _P, _I64, _I64]),
    "kdm_kernel_info": (C.c_int, [_P] + [C.POINTER(_I32)] * 5),
}


_bind = Binding("libksa_demod.so", "kdm_", ABI_VERSION, SIGNATURES)
LIB_PATH = _bind.path
load, lib, check = _bind.load, _bind.lib, _bind.check


def demod_taps(decim, taps_per_phase=8, cutoff=0.8, window="hamming", gain=1.0, deemph_us=None, sampling_rate=None,
               dc_block=False):
    """float32 [decim * taps_per_phase]: the low-pass of ddc_lowpass scaled to DC gain `gain`.  With deemph_us it is convolved
    with the single-pole response of time constant deemph_us microseconds at sampling_rate (the detector's rate) and cut to the
    same length: FM de-emphasis lives in the taps, not in a recursive kernel.  With dc_block the mean of the taps is subtracted,
    which removes the AM carrier."""
    decim, taps_per_phase = int(decim), int(taps_per_phase)
    n = decim * taps_per_phase
    if not (1 <= decim <= MAX_DECIM and taps_per_phase >= 1 and n <= MAX_TAPS and 0 < cutoff <= 1 and np.isfinite(gain)):
        raise KsaError("demod_taps wants decim 1..%d, decim * taps_per_phase 1..%d, 0 < cutoff <= 1 and a finite gain"
                       % (MAX_DECIM, MAX_TAPS))
    h = ddc_lowpass(decim, taps_per_phase, cutoff, window).astype(np.float64)
    if deemph_us is not None:
        if sampling_rate is None or not (deemph_us > 0 and sampling_rate > 0):
            raise KsaError("demod_taps wants deemph_us > 0 together with sampling_rate > 0")
        a = np.exp(-1.0 / (deemph_us * 1e-6 * sampling_rate))        # y[n] = (1 - a) x[n] + a y[n-1]
        h = np.convolve(h, (1 - a) * a ** np.arange(n))[:n]
    h = h * (gain / h.sum())
    if dc_block:
        h = h - h.mean()
    return h.astype(np.float32)


def write_wav(path, pcm_int16, rate):
    """A mono 16-bit WAV file of the int16 samples at `rate` samples per second."""
    pcm = np.ascontiguousarray(pcm_int16)
    if pcm.dtype != np.int16:
        raise KsaError("write_wav wants int16 samples, got %s" % pcm.dtype)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(rate))
        w.writeframes(pcm.reshape(-1).astype("<i2").tobytes())


class Demodulator(Companion):
    """Detector (mode "am" | "fm" | "pm"), real FIR low-pass and decimator by `decim` for one complex64 IQ stream on one GPU;
    the contract is include/ksa_demod.h.  out_fmt "f32" gives float32 outputs, "s16" int16 PCM of y * pcm_scale."""
    _binding, _info_fields = _bind, ("threads", "lds_bytes", "vgprs", "grid", "tile_out")

    def __init__(self, mode, decim, taps, out_fmt="f32", pcm_scale=32767.0, max_in=1 << 20, device=0, stream=None):
        if isinstance(mode, str) and mode.lower() not in MODES:
            raise KsaError("unknown mode [%s], expected one of %s" % (mode, "|".join(MODES)))
        if isinstance(out_fmt, str) and out_fmt.lower() not in OUT_FMTS:
            raise KsaError("unknown out_fmt [%s], expected one of %s" % (out_fmt, "|".join(OUT_FMTS)))
        self.mode = MODES[mode.lower()] if isinstance(mode, str) else int(mode)
        self.out_fmt = OUT_FMTS[out_fmt.lower()] if isinstance(out_fmt, str) else int(out_fmt)
        self.decim, self.device, self.max_in, self.pcm_scale = int(decim), int(device), int(max_in), float(pcm_scale)
        self.taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        self.ntaps = int(self.taps.size)
        self.lead = 1 if self.mode == MODE_FM else 0
        self.dtype = np.dtype(np.int16 if self.out_fmt == OUT_S16 else np.float32)
        self._create(self.device, self.mode, self.decim, self.ntaps, _ptr(self.taps), self.out_fmt, self.pcm_scale, self.max_in,
                     stream=stream)
        p, cap = C.c_void_p(), C.c_int64()
        check(lib().kdm_out_dev(self._h, C.byref(p), C.byref(cap)))
        self._out, self.out_capacity = p.value, cap.value

    # -- the stream form ----------------------------------------------------------------------------
    def out_count(self, n_in):
        n = C.c_int64()
        check(lib().kdm_out_count(self._h, int(n_in), C.byref(n)))
        return n.value

    def process_dev(self, iq, n_in, out=None, out_capacity=0):
        """The stream's next n_in complex64 samples from device memory; asynchronous.  out: a device buffer of out_capacity
        values (float32 or int16), or None for the object's own (self.out).  Returns the number of outputs."""
        n = C.c_int64()
        check(lib().kdm_process_dev(self._h, _ptr(iq), int(n_in), _ptr(out), int(out_capacity), C.byref(n)))
        return n.value

    def process(self, samples):
        """The stream's next samples from host memory (complex64 [n]); float32 or int16 outputs; synchronises."""
        a = np.ascontiguousarray(samples, dtype=np.complex64).reshape(-1)
        out = np.empty(self.out_count(a.size), dtype=self.dtype)
        n = C.c_int64()
        check(lib().kdm_process(self._h, _ptr(a), a.size, _ptr(out), out.size, C.byref(n)))
        return out[:n.value]

    # -- the block form -----------------------------------------------------------------------------
    def block_out_count(self, block_len):
        return (int(block_len) - self.lead - self.ntaps) // self.decim + 1

    def blocks_dev(self, iq, nblocks, block_len, block_stride=None, out=None, out_stride=None):
        """nblocks independent captures of block_len complex64 samples, block b at iq + b*block_stride samples (device
        memory); asynchronous.  out None: the object's own buffer at stride M.  Returns M, the outputs per block."""
        m = self.block_out_count(block_len)
        stride = int(block_len) if block_stride is None else int(block_stride)
        check(lib().kdm_blocks_dev(self._h, _ptr(iq), stride, int(nblocks), int(block_len), _ptr(out),
                                   m if out_stride is None else int(out_stride)))
        return m

    def read_out(self, count, first=0):
        """Values [first, first + count) of the object's output buffer as a numpy array; synchronises."""
        out = np.empty(max(int(count), 0), dtype=self.dtype)
        check(lib().kdm_read_out(self._h, _ptr(out), int(first), int(count)))
        return out

    # -- state --------------------------------------------------------------------------------------
    def set_taps(self, taps):
        """Replace the taps (the same count); the history is kept.  Synchronises."""
        t = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        if t.size != self.ntaps:
            raise KsaError("set_taps wants [%d] float32, got %s" % (self.ntaps, t.shape))
        check(lib().kdm_set_taps(self._h, _ptr(t)))
        self.taps = t

    def reset(self):
        check(lib().kdm_reset(self._h))

    def state(self):
        """dict(samples_in, samples_out) of the stream."""
        a, b = C.c_int64(), C.c_int64()
        check(lib().kdm_state(self._h, C.byref(a), C.byref(b)))
        return {"samples_in": a.value, "samples_out": b.value}

    @property
    def out(self):
        """The object's output buffer, float32 or int16 [out_capacity], for torch.as_tensor."""
        return DevArray(self._out, (self.out_capacity,), self, "<i2" if self.out_fmt == OUT_S16 else "<f4")
