"""Rational (polyphase L / M) resampler on the GPU: ctypes binding of include/ksa_resamp.h (libksa_resamp.so, a companion of
libksa.so) and the Resampler class over it.  Real float32 (what the demodulator leaves) or complex64 (what the down-converter
and the channelizer leave) in device memory becomes the same signal at L / M times the rate, so that the output rate no longer
has to be the capture rate over a whole number.  There is no fallback: a missing library raises."""
import ctypes as C
import math

import numpy as np

from ._companion import Binding, Companion
from ._lib import KsaError
from .engine import DevArray, _ptr

ABI_VERSION = 1
TYPE_F32, TYPE_C64 = 0, 1
TYPES = {"f32": TYPE_F32, "c64": TYPE_C64}
OUT_SAME, OUT_S16 = 0, 1
OUT_FMTS = {"same": OUT_SAME, "s16": OUT_S16}
MAX_L, MAX_M, MAX_RATIO, MAX_PHASE_TAPS, MAX_TAPS, MAX_IN, MAX_POSITION = 1024, 16384, 16, 256, 16384, 2 ** 28 - 1, 2 ** 52

_P = C.c_void_p
_I32, _I64, _F = C.c_int32, C.c_int64, C.c_float

# name -> (restype, argtypes); every symbol include/ksa_resamp.h declares
SIGNATURES = {
    "krs_abi_version": (C.c_int, []),
    "krs_last_error": (C.c_char_p, []),
    "krs_create": (C.c_int, [_I32, _I32, _I32, _I32, _I32, _P, _I32, _F, _I64, C.POINTER(_P)]),
    "krs_destroy": (None, [_P]),
    "krs_set_stream": (C.c_int, [_P, _P]),
    "krs_synchronize": (C.c_int, [_P]),
    "krs_out_count": (C.c_int, [_P, _I64, C.POINTER(_I64)]),
    "krs_process_dev": (C.c_int, [_P, _P, _I64, _P, _I64, C.POINTER(_I64)]),
    "krs_process": (C.c_int, [_P, _P, _I64, _P, _I64, C.POINTER(_I64)]),
    "krs_blocks_dev": (C.c_int, [_P, _P, _I64, _I64, _I64, _P, _I64]),
    "krs_set_taps": (C.c_int, [_P, _P]),
    "krs_reset": (C.c_int, [_P]),
    "krs_reset_at": (C.c_int, [_P, _I64]),
    "krs_state": (C.c_int, [_P, C.POINTER(_I64), C.POINTER(_I64)]),
    "krs_out_dev": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_I64)]),
    "krs_read_out": (C.c_int, [_P, _P, _I64, _I64]),
    "krs_kernel_info": (C.c_int, [_P] + [C.POINTER(_I32)] * 5),
}


_bind = Binding("libksa_resamp.so", "krs_", ABI_VERSION, SIGNATURES)
LIB_PATH = _bind.path
load, lib, check = _bind.load, _bind.lib, _bind.check


def _pair_ok(L, M):
    return 1 <= L <= MAX_L and 1 <= M <= MAX_M and M <= MAX_RATIO * L


def rate_ratio(rate_in, rate_out):
    """The reduced (L, M) with rate_out = rate_in * L / M.  Both rates are whole numbers of Hz."""
    try:
        ok = float(rate_in) == int(rate_in) and float(rate_out) == int(rate_out) and rate_in >= 1 and rate_out >= 1
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise KsaError("rate_ratio wants two whole rates >= 1, got [%s] and [%s]" % (rate_in, rate_out))
    a, b = int(rate_out), int(rate_in)
    g = math.gcd(a, b)
    L, M = a // g, b // g
    if not _pair_ok(L, M):
        raise KsaError("rate_ratio: [%s] -> [%s] is L / M = %d / %d, outside L 1..%d, M 1..%d, M <= %d L"
                       % (rate_in, rate_out, L, M, MAX_L, MAX_M, MAX_RATIO))
    return L, M


def resample_taps(L, M, taps_per_phase=8):
    """float32 [L * P], P = taps_per_phase * ceil(max(L, M) / L): a Hamming-windowed sinc at the zero-stuffed rate with its
    cut-off at 0.8 of the narrower Nyquist band, h = sinc(0.8 t / max(L, M)) * hamming(T) over t = k - (T - 1) / 2, scaled
    to sum L (DC gain 1 after zero-stuffing by L)."""
    L, M, tpp = int(L), int(M), int(taps_per_phase)
    if not (_pair_ok(L, M) and tpp >= 1):
        raise KsaError("resample_taps wants L 1..%d, M 1..%d with M <= %d L and taps_per_phase >= 1" % (MAX_L, MAX_M, MAX_RATIO))
    W = max(L, M)
    P = tpp * -(-W // L)
    T = L * P
    if P > MAX_PHASE_TAPS or T > MAX_TAPS:
        raise KsaError("resample_taps: L %d, M %d, taps_per_phase %d need %d taps per phase (limit %d) and %d taps (limit %d)"
                       % (L, M, tpp, P, MAX_PHASE_TAPS, T, MAX_TAPS))
    t = np.arange(T, dtype=np.float64) - (T - 1) / 2
    h = np.sinc(0.8 * t / W) * np.hamming(T)
    return (h * (L / h.sum())).astype(np.float32)


class Resampler(Companion):
    """Polyphase L / M resampler for one stream of real float32 (type "f32") or complex64 (type "c64") samples on one GPU;
    the contract is include/ksa_resamp.h.  taps: float32 [L * P].  out_fmt "same" gives the input's type, "s16" int16 PCM of
    y * pcm_scale (real input only)."""
    _binding, _info_fields = _bind, ("threads", "lds_bytes", "vgprs", "grid", "tile_out")

    def __init__(self, L, M, taps, type="f32", out_fmt="same", pcm_scale=32767.0, max_in=1 << 20, device=0, stream=None):
        if isinstance(type, str) and type.lower() not in TYPES:
            raise KsaError("unknown type [%s], expected one of %s" % (type, "|".join(TYPES)))
        if isinstance(out_fmt, str) and out_fmt.lower() not in OUT_FMTS:
            raise KsaError("unknown out_fmt [%s], expected one of %s" % (out_fmt, "|".join(OUT_FMTS)))
        self.type = TYPES[type.lower()] if isinstance(type, str) else int(type)
        self.out_fmt = OUT_FMTS[out_fmt.lower()] if isinstance(out_fmt, str) else int(out_fmt)
        self.L, self.M, self.device, self.max_in, self.pcm_scale = int(L), int(M), int(device), int(max_in), float(pcm_scale)
        self.taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        if self.L < 1 or self.taps.size % self.L or self.taps.size == 0:
            raise KsaError("Resampler wants L >= 1 and a whole number of taps per phase, got L %d and %d taps" % (self.L, self.taps.size))
        self.taps_per_phase = int(self.taps.size) // self.L
        self.in_dtype = np.dtype(np.complex64 if self.type == TYPE_C64 else np.float32)
        self.dtype = np.dtype(np.int16) if self.out_fmt == OUT_S16 else self.in_dtype
        self._create(self.device, self.type, self.L, self.M, self.taps_per_phase, _ptr(self.taps), self.out_fmt, self.pcm_scale,
                     self.max_in, stream=stream)
        p, cap = C.c_void_p(), C.c_int64()
        check(lib().krs_out_dev(self._h, C.byref(p), C.byref(cap)))
        self._out, self.out_capacity = p.value, cap.value

    # -- the stream form ----------------------------------------------------------------------------
    def out_count(self, n_in):
        n = C.c_int64()
        check(lib().krs_out_count(self._h, int(n_in), C.byref(n)))
        return n.value

    def process_dev(self, x, n_in, out=None, out_capacity=0):
        """The stream's next n_in samples from device memory; asynchronous.  out: a device buffer of out_capacity values, or
        None for the object's own (self.out).  Returns the number of outputs."""
        n = C.c_int64()
        check(lib().krs_process_dev(self._h, _ptr(x), int(n_in), _ptr(out), int(out_capacity), C.byref(n)))
        return n.value

    def process(self, samples):
        """The stream's next samples from host memory (float32 or complex64 [n]); synchronises."""
        a = np.ascontiguousarray(samples, dtype=self.in_dtype).reshape(-1)
        out = np.empty(self.out_count(a.size), dtype=self.dtype)
        n = C.c_int64()
        check(lib().krs_process(self._h, _ptr(a), a.size, _ptr(out), out.size, C.byref(n)))
        return out[:n.value]

    # -- the block form -----------------------------------------------------------------------------
    def block_first(self):
        """The first output of a block that is kept: ceil((P - 1) L / M)."""
        return -(-(self.taps_per_phase - 1) * self.L // self.M)

    def block_out_count(self, block_len):
        """J = ceil(block_len L / M) - first; below 1 the call is refused."""
        return -(-int(block_len) * self.L // self.M) - self.block_first()

    def blocks_dev(self, x, nblocks, block_len, block_stride=None, out=None, out_stride=None):
        """nblocks independent blocks of block_len samples, block b at x + b*block_stride samples (device memory);
        asynchronous.  out None: the object's own buffer at stride J.  Returns J, the outputs per block."""
        j = self.block_out_count(block_len)
        stride = int(block_len) if block_stride is None else int(block_stride)
        check(lib().krs_blocks_dev(self._h, _ptr(x), stride, int(nblocks), int(block_len), _ptr(out),
                                   j if out_stride is None else int(out_stride)))
        return j

    def read_out(self, count, first=0):
        """Values [first, first + count) of the object's output buffer as a numpy array; synchronises."""
        out = np.empty(max(int(count), 0), dtype=self.dtype)
        check(lib().krs_read_out(self._h, _ptr(out), int(first), int(count)))
        return out

    # -- state --------------------------------------------------------------------------------------
    def set_taps(self, taps):
        """Replace the taps (the same count); the history is kept.  Synchronises."""
        t = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        if t.size != self.taps.size:
            raise KsaError("set_taps wants [%d] float32, got %s" % (self.taps.size, t.shape))
        check(lib().krs_set_taps(self._h, _ptr(t)))
        self.taps = t

    def reset(self):
        check(lib().krs_reset(self._h))

    def reset_at(self, samples_in):
        """Zero history, counts as if samples_in zero samples had been fed."""
        check(lib().krs_reset_at(self._h, int(samples_in)))

    def state(self):
        """dict(samples_in, samples_out) of the stream."""
        a, b = C.c_int64(), C.c_int64()
        check(lib().krs_state(self._h, C.byref(a), C.byref(b)))
        return {"samples_in": a.value, "samples_out": b.value}

    @property
    def out(self):
        """The object's output buffer [out_capacity], for torch.as_tensor."""
        return DevArray(self._out, (self.out_capacity,), self, {"int16": "<i2", "float32": "<f4", "complex64": "<c8"}[self.dtype.name])
