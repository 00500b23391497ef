"""Frequency-mask trigger and per-bin occupancy counter on the GPU: ctypes binding of include/ksa_mask.h (libksa_mask.so, a
companion of libksa.so) and the SpectrumMask class over it.  Every spectrum is compared against an upper and a lower limit
line; the frames that cross a line are reported (which, where, by how much) and every bin counts the spectra that crossed.  It
consumes the per-frame dB rows the engine already writes to device memory (frames_dev(cur_db=...),
curscan_dev(out_mode=OUT_DB)).  There is no fallback: a missing library raises."""
import ctypes as C

import numpy as np

from ._companion import Binding, Companion
from ._lib import KsaError
from .engine import DevArray, _ptr

ABI_VERSION = 1
MAX_CAPACITY = 1 << 20

_P = C.c_void_p
_I32, _I64 = C.c_int32, C.c_int64

# the 32 bytes of ksm_event
EVENT_DTYPE = np.dtype([("row", "<i8"), ("nover", "<i4"), ("nunder", "<i4"), ("nnan", "<i4"), ("peak_bin", "<i4"),
                        ("peak_excess", "<f4"), ("peak_kind", "<i4")])
assert EVENT_DTYPE.itemsize == 32

# name -> (restype, argtypes); every symbol include/ksa_mask.h declares
SIGNATURES = {
    "ksm_abi_version": (C.c_int, []),
    "ksm_last_error": (C.c_char_p, []),
    "ksm_create": (C.c_int, [_I32, _I32, _P, _P, _I32, _I32, C.POINTER(_P)]),
    "ksm_destroy": (None, [_P]),
    "ksm_set_stream": (C.c_int, [_P, _P]),
    "ksm_synchronize": (C.c_int, [_P]),
    "ksm_check_rows_dev": (C.c_int, [_P, _P, _I64, _I64, _P]),
    "ksm_check_rows": (C.c_int, [_P, _P, _I64]),
    "ksm_set_mask": (C.c_int, [_P, _P, _P]),
    "ksm_set_row_base": (C.c_int, [_P, _I64]),
    "ksm_read_hits": (C.c_int, [_P, _P, C.POINTER(_I64)]),
    "ksm_read_events": (C.c_int, [_P, _P, _I64, C.POINTER(_I64), C.POINTER(_I64)]),
    "ksm_hits_dev": (C.c_int, [_P, C.POINTER(_P)]),
    "ksm_events_dev": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P)]),
    "ksm_merge_hits_dev": (C.c_int, [_P, _P, _I64]),
    "ksm_clear_events": (C.c_int, [_P]),
    "ksm_reset": (C.c_int, [_P]),
    "ksm_kernel_info": (C.c_int, [_P] + [C.POINTER(_I32)] * 5),
}


_bind = Binding("libksa_mask.so", "ksm_", ABI_VERSION, SIGNATURES)
LIB_PATH = _bind.path
load, lib, check = _bind.load, _bind.lib, _bind.check


def learn_mask(rows, margin_db):
    """float32 [nbins]: the largest value every bin took in rows [k][nbins] (NaNs skipped) plus margin_db, in float32.  A bin
    that is NaN in every row becomes +inf, which disables the line there."""
    r = np.asarray(rows, dtype=np.float32)
    r = r.reshape(-1, r.shape[-1])
    with np.errstate(invalid="ignore"):
        up = (np.fmax.reduce(r, axis=0) + np.float32(margin_db)).astype(np.float32)
    up[np.isnan(up)] = np.inf
    return up


def _line(values, nbins, name):
    a = np.ascontiguousarray(values, dtype=np.float32)
    if a.ndim == 0:
        a = np.full(nbins, a, dtype=np.float32)
    if a.shape != (nbins,):
        raise KsaError("%s line wants [%d] float32, got %s" % (name, nbins, a.shape))
    return a


class SpectrumMask(Companion):
    """An upper and a lower limit line over nbins bins on one GPU, int64 hits[3][nbins] (over, under, NaN) and the first
    `capacity` event records in ascending row order.  A row is an event when at least min_bins of its bins crossed a line or
    any is NaN.  The float32 rule is stated in include/ksa_mask.h."""
    _binding, _info_fields = _bind, ("threads", "lds_bytes", "vgprs", "grid", "vec")

    def __init__(self, nbins, upper, lower=None, min_bins=1, capacity=4096, device=0, stream=None):
        self.nbins = int(nbins)
        self.min_bins, self.capacity, self.device = int(min_bins), int(capacity), int(device)
        self.upper = _line(upper, self.nbins, "upper")
        self.lower = None if lower is None else _line(lower, self.nbins, "lower")
        self._create(self.device, self.nbins, _ptr(self.upper), None if self.lower is None else _ptr(self.lower),
                     self.min_bins, self.capacity, stream=stream)

    # -- checking ---------------------------------------------------------------------------------
    def check_rows_dev(self, rows, nrows=None, row_stride=None, row_event=None):
        """nrows float32 rows from device memory (a torch tensor, DevArray pointer or int address), row i at
        rows + i*row_stride floats; asynchronous on the object's stream.  nrows defaults to the first dimension of a 2-D
        tensor.  row_event: device uint8 [nrows] that receives 1 where the row is an event."""
        if nrows is None:
            shape = getattr(rows, "shape", None)
            if shape is None or len(shape) != 2:
                raise KsaError("check_rows_dev needs nrows unless rows is a 2-D tensor")
            nrows = shape[0]
        stride = self.nbins if row_stride is None else int(row_stride)
        check(lib().ksm_check_rows_dev(self._h, _ptr(rows), stride, int(nrows), None if row_event is None else _ptr(row_event)))

    def check_rows(self, host_rows):
        """float32 [k][nbins] (or one row) from host memory; synchronises."""
        a = np.ascontiguousarray(host_rows, dtype=np.float32)
        if a.size % self.nbins or (a.ndim > 1 and a.shape[-1] != self.nbins):
            raise KsaError("check_rows wants [k][%d] float32, got %s" % (self.nbins, a.shape))
        if a.size:
            check(lib().ksm_check_rows(self._h, _ptr(a), a.size // self.nbins))

    def set_mask(self, upper, lower=None):
        """Replace the lines; hits, rows_seen and events are kept.  Synchronises."""
        up = _line(upper, self.nbins, "upper")
        lo = None if lower is None else _line(lower, self.nbins, "lower")
        check(lib().ksm_set_mask(self._h, _ptr(up), None if lo is None else _ptr(lo)))
        self.upper, self.lower = up, lo

    def set_row_base(self, row_base):
        """The index the next row gets (and rows_seen)."""
        if not -2 ** 63 <= int(row_base) < 2 ** 63:
            raise KsaError("set_row_base(%d): outside int64" % row_base)
        check(lib().ksm_set_row_base(self._h, int(row_base)))

    def merge_hits_dev(self, hits, rows_seen_add=0):
        """hits += another object's hits in device memory (int64 [3][nbins])."""
        check(lib().ksm_merge_hits_dev(self._h, _ptr(hits), int(rows_seen_add)))

    def clear_events(self):
        check(lib().ksm_clear_events(self._h))

    def reset(self):
        check(lib().ksm_reset(self._h))

    # -- results ----------------------------------------------------------------------------------
    def hits(self):
        """(int64 [3, nbins]: over, under, NaN; rows_seen); synchronises."""
        out = np.empty((3, self.nbins), dtype=np.int64)
        seen = C.c_int64()
        check(lib().ksm_read_hits(self._h, _ptr(out), C.byref(seen)))
        return out, seen.value

    @property
    def rows_seen(self):
        seen = C.c_int64()
        check(lib().ksm_read_hits(self._h, None, C.byref(seen)))
        return seen.value

    def occupancy(self):
        """float64 [nbins]: the share of the rows seen in which the bin crossed a line; 0 when no rows were seen."""
        h, seen = self.hits()
        if seen <= 0:
            return np.zeros(self.nbins, dtype=np.float64)
        return (h[0] + h[1]).astype(np.float64) / seen

    def events(self):
        """(structured array of EVENT_DTYPE: the stored events in ascending row order; events_total); synchronises."""
        out = np.zeros(self.capacity, dtype=EVENT_DTYPE)
        stored, total = C.c_int64(), C.c_int64()
        check(lib().ksm_read_events(self._h, _ptr(out), self.capacity, C.byref(stored), C.byref(total)))
        return out[:stored.value].copy(), total.value

    def hits_view(self):
        p = C.c_void_p()
        check(lib().ksm_hits_dev(self._h, C.byref(p)))
        return DevArray(p.value, (3, self.nbins), self, "<i8")
