"""Spectrum density (persistence) histogram on the GPU: ctypes binding of include/ksa_density.h (libksa_density.so, the
companion of libksa.so) and the SpectrumDensity class over it.  A bitmap of level against frequency, each cell counting how
many spectra passed through that level at that frequency; it consumes the per-frame dB rows the engine already writes to
device memory (frames_dev(cur_db=...), curscan_dev(out_mode=OUT_DB)).  There is no fallback: a missing library raises."""
import ctypes as C

import numpy as np

from ._companion import Binding, Companion
from ._lib import KsaError
from .engine import DevArray, _ptr

ABI_VERSION = 1

_P = C.c_void_p
_I32, _I64 = C.c_int32, C.c_int64

# name -> (restype, argtypes); every symbol include/ksa_density.h declares
SIGNATURES = {
    "ksd_abi_version": (C.c_int, []),
    "ksd_last_error": (C.c_char_p, []),
    "ksd_create": (C.c_int, [_I32, _I32, _I32, _I32, C.c_float, C.c_float, C.POINTER(_P)]),
    "ksd_destroy": (None, [_P]),
    "ksd_set_stream": (C.c_int, [_P, _P]),
    "ksd_synchronize": (C.c_int, [_P]),
    "ksd_add_rows_dev": (C.c_int, [_P, _P, _I64, _I64]),
    "ksd_add_rows": (C.c_int, [_P, _P, _I64]),
    "ksd_decay": (C.c_int, [_P, _I64, _I64]),
    "ksd_merge_dev": (C.c_int, [_P, _P, _I64]),
    "ksd_reset": (C.c_int, [_P]),
    "ksd_read": (C.c_int, [_P, _P, C.POINTER(_I64)]),
    "ksd_counts_dev": (C.c_int, [_P, C.POINTER(_P)]),
    "ksd_kernel_info": (C.c_int, [_P] + [C.POINTER(_I32)] * 6),
}


_bind = Binding("libksa_density.so", "ksd_", ABI_VERSION, SIGNATURES)
LIB_PATH = _bind.path
load, lib, check = _bind.load, _bind.lib, _bind.check


class SpectrumDensity(Companion):
    """int64 counts[levels + 1][width] on one GPU: row k < levels counts the dB values in [lo + k*step, lo + (k+1)*step) (the
    first and last level also take what lies below and above the range), the extra last row counts NaNs; width must divide
    nbins and nbins / width adjacent bins share a column.  The float32 rule is stated in include/ksa_density.h."""
    _binding, _info_fields = _bind, ("threads", "lds_bytes", "vgprs", "grid", "strip_cols", "lds_optin")

    def __init__(self, nbins, width=None, levels=256, lo_db=-140.0, hi_db=0.0, device=0, stream=None):
        self.nbins = int(nbins)
        self.width = self.nbins if width is None else int(width)
        self.levels = int(levels)
        self.lo_db, self.hi_db = float(lo_db), float(hi_db)
        self.device = int(device)
        self._create(self.device, self.nbins, self.width, self.levels, self.lo_db, self.hi_db, stream=stream)

    # -- counting ---------------------------------------------------------------------------------
    def add_rows_dev(self, rows, nrows, row_stride=None):
        """nrows float32 rows from device memory (a torch tensor, DevArray pointer or int address), row i at
        rows + i*row_stride floats; asynchronous on the object's stream."""
        stride = self.nbins if row_stride is None else int(row_stride)
        check(lib().ksd_add_rows_dev(self._h, _ptr(rows), stride, int(nrows)))

    def add_rows(self, host_rows):
        """float32 [k][nbins] (or one row) from host memory; synchronises."""
        a = np.ascontiguousarray(host_rows, dtype=np.float32)
        if a.size % self.nbins or (a.ndim > 1 and a.shape[-1] != self.nbins):
            raise KsaError("add_rows wants [k][%d] float32, got %s" % (self.nbins, a.shape))
        if a.size:
            check(lib().ksd_add_rows(self._h, _ptr(a), a.size // self.nbins))

    def decay(self, num, den):
        """Every count becomes floor(count * num / den), 0 <= num <= den < 2^31; rows_seen stays."""
        if not (-2 ** 63 <= int(num) < 2 ** 63 and -2 ** 63 <= int(den) < 2 ** 63):
            raise KsaError("decay(%d, %d): outside int64" % (num, den))
        check(lib().ksd_decay(self._h, int(num), int(den)))

    def merge_dev(self, counts, rows_seen_add=0):
        """counts += another histogram of the same shape in device memory (int64 [levels + 1][width])."""
        check(lib().ksd_merge_dev(self._h, _ptr(counts), int(rows_seen_add)))

    def reset(self):
        check(lib().ksd_reset(self._h))

    def read(self):
        """(counts int64 [levels + 1, width], rows_seen); synchronises."""
        out = np.empty((self.levels + 1, self.width), dtype=np.int64)
        seen = C.c_int64()
        check(lib().ksd_read(self._h, _ptr(out), C.byref(seen)))
        return out, seen.value

    @property
    def rows_seen(self):
        seen = C.c_int64()
        check(lib().ksd_read(self._h, None, C.byref(seen)))
        return seen.value

    def counts_dev(self):
        p = C.c_void_p()
        check(lib().ksd_counts_dev(self._h, C.byref(p)))
        return DevArray(p.value, (self.levels + 1, self.width), self, "<i8")

    # -- host helpers -----------------------------------------------------------------------------
    def level_edges(self):
        """float64 [levels + 1]: lo + k*(hi - lo)/levels, the nominal edges of the levels (the float32 rule decides hits)."""
        return level_edges(self.levels, self.lo_db, self.hi_db)

    @staticmethod
    def image(counts, normalize="column", log=False):
        return image(counts, normalize, log)


def level_edges(levels, lo_db, hi_db):
    return lo_db + np.arange(levels + 1, dtype=np.float64) * (hi_db - lo_db) / levels


def image(counts, normalize="column", log=False):
    """float32 [levels, width] in 0..1 from counts [levels + 1, width] (the NaN row dropped, level 0 first): ready for
    imshow(origin="lower").  normalize "column": each column by its own largest cell (a weak burst beside a strong carrier
    stays visible); "max": by the largest cell of the bitmap.  log: log1p of the counts first."""
    c = np.asarray(counts)[:-1].astype(np.float64)
    if log:
        c = np.log1p(c)
    if normalize == "column":
        top = c.max(axis=0, keepdims=True)
    elif normalize == "max":
        top = np.full((1, c.shape[1]), c.max() if c.size else 0.0)
    else:
        raise KsaError("image: normalize [%s] is neither column nor max" % normalize)
    return (c / np.where(top > 0, top, 1.0)).astype(np.float32)
