"""DC-offset and IQ-imbalance corrector on the GPU: ctypes binding of include/ksa_iqfix.h (libksa_iqfix.so, a companion of
libksa.so) and the IqCorrector class over it.  Raw IQ in device memory is corrected into complex64 in one pass, and the same
pass accumulates the five integer sums the correction is solved from on the host.  There is no fallback: a missing library
raises."""
import ctypes as C
import math

import numpy as np

from ._companion import FORMATS, SAMPLE_DTYPES, Binding, Companion, format_of
from ._lib import KsaError, FMT_C64, FMT_U8, FMT_S8, FMT_S16
from .engine import DevArray, _ptr

ABI_VERSION = 1
MAX_IN, MAX_COUNT, UNIT = 2 ** 28 - 1, 1 << 30, 1 << 30
MODE_DC, MODE_IQ = 1, 2
FLAG_DEGENERATE, FLAG_EMPTY = 1, 2
MODES = {"dc": MODE_DC, "iq": MODE_IQ, "dc+iq": MODE_DC | MODE_IQ}

_P = C.c_void_p
_I32, _I64, _F = C.c_int32, C.c_int64, C.c_float


class Coeffs(C.Structure):
    """kqf_coeffs: 32 bytes, no padding."""
    _fields_ = [("dc_i", _F), ("dc_q", _F), ("c", _F), ("d", _F), ("flags", _I32), ("mode", _I32), ("count", _I64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


assert C.sizeof(Coeffs) == 32

# name -> (restype, argtypes); every symbol include/ksa_iqfix.h declares
SIGNATURES = {
    "kqf_abi_version": (C.c_int, []),
    "kqf_last_error": (C.c_char_p, []),
    "kqf_create": (C.c_int, [_I32, _I32, _F, _F, _I64, C.POINTER(_P)]),
    "kqf_destroy": (None, [_P]),
    "kqf_set_stream": (C.c_int, [_P, _P]),
    "kqf_synchronize": (C.c_int, [_P]),
    "kqf_blocks_dev": (C.c_int, [_P, _P, _I64, _I64, _I64, _P, _I64, _I32]),
    "kqf_accumulate_dev": (C.c_int, [_P, _P, _I64, _I64, _I64]),
    "kqf_apply": (C.c_int, [_P, _P, _I64, _P, _I32]),
    "kqf_solve": (C.c_int, [_P, _I32, C.POINTER(Coeffs)]),
    "kqf_set_coeffs": (C.c_int, [_P, _F, _F, _F, _F]),
    "kqf_get_coeffs": (C.c_int, [_P, C.POINTER(Coeffs)]),
    "kqf_read_stats": (C.c_int, [_P, C.POINTER(_I64)]),
    "kqf_stats_dev": (C.c_int, [_P, C.POINTER(_P)]),
    "kqf_clear_stats": (C.c_int, [_P]),
    "kqf_out_dev": (C.c_int, [_P, C.POINTER(_P)]),
    "kqf_kernel_info": (C.c_int, [_P] + [C.POINTER(_I32)] * 5),
}


_bind = Binding("libksa_iqfix.so", "kqf_", ABI_VERSION, SIGNATURES)
LIB_PATH = _bind.path
load, lib, check = _bind.load, _bind.lib, _bind.check


def imbalance_of(c, d):
    """(gain error in dB, phase error in degrees) read off the correction's Q row (c, d): gain = 1 / hypot(c, d) and phase =
    atan2(-c, d).  For a receiver whose Q is g (I sin(phi) + Q cos(phi)) the solve gives c = -tan(phi) and d = 1 / (g cos(phi)),
    so the two figures are g and phi to first order in the error (1 dB and 5 degrees read 0.92 dB and 5.6 degrees)."""
    c, d = float(c), float(d)
    return 20.0 * math.log10(1.0 / math.hypot(c, d)), math.degrees(math.atan2(-c, d))


class IqCorrector(Companion):
    """A DC-offset and IQ-imbalance corrector on one GPU; the contract is include/ksa_iqfix.h.  fmt: c64 | u8 | s8 | s16 (or
    the number); max_in: the largest number of samples per call.  It starts with the identity coefficients and zero sums."""
    _binding, _info_fields = _bind, ("threads", "lds_bytes", "vgprs", "grid", "tile")

    def __init__(self, fmt="c64", max_in=1 << 20, u8_offset=127.5, u8_scale=127.5, device=0, stream=None):
        self.fmt = format_of(fmt)
        self.max_in, self.device = int(max_in), int(device)
        self.in_dtype = SAMPLE_DTYPES.get(self.fmt, np.dtype(np.complex64))
        self._create(self.device, self.fmt, float(u8_offset), float(u8_scale), self.max_in, stream=stream)

    # -- the pass -----------------------------------------------------------------------------------
    def blocks_dev(self, iq, nblocks, block_len, block_stride=None, out=None, out_stride=None, accumulate=False):
        """nblocks blocks of block_len samples, block b at iq + b*block_stride samples (device memory), corrected into out
        (device complex64, block b at b*out_stride) or, with out None, into the object's own packed buffer; with accumulate
        the raw samples also enter the sums.  Asynchronous."""
        stride = int(block_len) if block_stride is None else int(block_stride)
        check(lib().kqf_blocks_dev(self._h, _ptr(iq), stride, int(nblocks), int(block_len), _ptr(out),
                                   int(block_len) if out_stride is None else int(out_stride), 1 if accumulate else 0))

    def accumulate_dev(self, iq, nblocks, block_len, block_stride=None):
        """The raw samples of the blocks into the sums; nothing else is written.  Asynchronous."""
        stride = int(block_len) if block_stride is None else int(block_stride)
        check(lib().kqf_accumulate_dev(self._h, _ptr(iq), stride, int(nblocks), int(block_len)))

    def apply(self, samples, accumulate=False):
        """One block from host memory (complex64 [n], or [n][2] of the integer formats); synchronises.  Returns complex64 [n]."""
        a = np.ascontiguousarray(samples, dtype=self.in_dtype)
        n = a.size if self.fmt == FMT_C64 else a.size // 2
        out = np.zeros(n, dtype=np.complex64)
        check(lib().kqf_apply(self._h, _ptr(a), n, _ptr(out), 1 if accumulate else 0))
        return out

    # -- coefficients -------------------------------------------------------------------------------
    def solve(self, mode="dc+iq"):
        """The sums into coefficients, which hold from the next call; synchronises.  mode: dc | iq | dc+iq (or the bits).
        Returns dict(dc_i, dc_q, c, d, flags, mode, count)."""
        if isinstance(mode, str) and mode.lower() not in MODES:
            raise KsaError("unknown mode [%s], expected one of %s" % (mode, "|".join(MODES)))
        co = Coeffs()
        check(lib().kqf_solve(self._h, MODES[mode.lower()] if isinstance(mode, str) else int(mode), C.byref(co)))
        return co.as_dict()

    def set_coeffs(self, dc_i=0.0, dc_q=0.0, c=0.0, d=1.0):
        check(lib().kqf_set_coeffs(self._h, float(dc_i), float(dc_q), float(c), float(d)))

    def get_coeffs(self):
        co = Coeffs()
        check(lib().kqf_get_coeffs(self._h, C.byref(co)))
        return co.as_dict()

    # -- sums ---------------------------------------------------------------------------------------
    def read_stats(self):
        """int64 [6]: the five sums and the count; synchronises."""
        s = np.zeros(6, dtype=np.int64)
        check(lib().kqf_read_stats(self._h, s.ctypes.data_as(C.POINTER(_I64))))
        return s

    def clear_stats(self):
        check(lib().kqf_clear_stats(self._h))

    def stats_view(self):
        """The six words in device memory, for torch.as_tensor."""
        p = C.c_void_p()
        check(lib().kqf_stats_dev(self._h, C.byref(p)))
        return DevArray(p.value, (6,), self, "<i8")

    # -- output -------------------------------------------------------------------------------------
    @property
    def out_ptr(self):
        """The device address of the object's own output buffer, complex64 [max_in]."""
        p = C.c_void_p()
        check(lib().kqf_out_dev(self._h, C.byref(p)))
        return p.value

    def out_view(self, n=None):
        """The first n values of the object's own output buffer (default all) as complex64 in device memory."""
        return DevArray(self.out_ptr, (self.max_in if n is None else int(n),), self, "<c8")
