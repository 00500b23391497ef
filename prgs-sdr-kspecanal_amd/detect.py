"""CFAR signal detector and emission list on the GPU: ctypes binding of include/ksa_detect.h (libksa_detect.so, a companion of
libksa.so) and the SignalDetector class over it.  Every bin of every spectrum is compared against a noise floor estimated from
the bins around it (cell averaging, greatest-of or smallest-of), the detected bins of a row are grouped into emissions (start
bin, stop bin, peak, floor) and every bin counts the rows in which it lay inside an emission.  It consumes the per-frame dB
rows the engine already writes to device memory (frames_dev(cur_db=...), curscan_dev(out_mode=OUT_DB)).  There is no fallback:
a missing library raises."""
import ctypes as C

import numpy as np

from ._companion import Binding, Companion
from ._lib import KsaError
from .engine import DevArray, _ptr

ABI_VERSION = 1
MIN_NBINS, MAX_NBINS = 16, 16384
MAX_TRAIN, MAX_GUARD, MAX_GAP = 1024, 256, 1024
MAX_CAPACITY = 1 << 20
MODES = {"ca": 0, "go": 1, "so": 2}

_P = C.c_void_p
_I32, _I64 = C.c_int32, C.c_int64

# the 32 bytes of kse_emission
EMISSION_DTYPE = np.dtype([("row", "<i8"), ("bin_lo", "<i4"), ("bin_hi", "<i4"), ("peak_bin", "<i4"), ("ndet", "<i4"),
                           ("peak_db", "<f4"), ("floor_db", "<f4")])
assert EMISSION_DTYPE.itemsize == 32

# name -> (restype, argtypes); every symbol include/ksa_detect.h declares
SIGNATURES = {
    "kse_abi_version": (C.c_int, []),
    "kse_last_error": (C.c_char_p, []),
    "kse_create": (C.c_int, [_I32, _I32, _I32, _I32, C.c_float, _I32, _I32, _I32, _I32, C.POINTER(_P)]),
    "kse_destroy": (None, [_P]),
    "kse_set_stream": (C.c_int, [_P, _P]),
    "kse_synchronize": (C.c_int, [_P]),
    "kse_detect_rows_dev": (C.c_int, [_P, _P, _I64, _I64, _P, _P]),
    "kse_detect_rows": (C.c_int, [_P, _P, _I64]),
    "kse_set_params": (C.c_int, [_P, _I32, _I32, C.c_float, _I32, _I32, _I32]),
    "kse_set_row_base": (C.c_int, [_P, _I64]),
    "kse_read_hits": (C.c_int, [_P, _P, C.POINTER(_I64)]),
    "kse_read_emissions": (C.c_int, [_P, _P, _I64, C.POINTER(_I64), C.POINTER(_I64)]),
    "kse_hits_dev": (C.c_int, [_P, C.POINTER(_P)]),
    "kse_emissions_dev": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P)]),
    "kse_merge_hits_dev": (C.c_int, [_P, _P, _I64]),
    "kse_clear_emissions": (C.c_int, [_P]),
    "kse_reset": (C.c_int, [_P]),
    "kse_kernel_info": (C.c_int, [_P] + [C.POINTER(_I32)] * 6),
}


_bind = Binding("libksa_detect.so", "kse_", ABI_VERSION, SIGNATURES)
LIB_PATH = _bind.path
load, lib, check = _bind.load, _bind.lib, _bind.check


def _mode(mode):
    if isinstance(mode, str):
        if mode.lower() not in MODES:
            raise KsaError("mode %r is none of ca, go, so" % mode)
        return MODES[mode.lower()]
    return int(mode)


def emission_freqs(ev, freqs):
    """(centre, width) in Hz, float64 [len(ev)] each, of the emission records ev from the bin frequencies freqs [nbins]
    (ascending, evenly spaced): the centre is the middle between the first and the last bin, the width counts whole bins."""
    f = np.asarray(freqs, dtype=np.float64)
    step = (f[-1] - f[0]) / (len(f) - 1) if len(f) > 1 else 0.0
    lo, hi = f[ev["bin_lo"]], f[ev["bin_hi"]]
    return (lo + hi) / 2, (ev["bin_hi"] - ev["bin_lo"] + 1) * step


class SignalDetector(Companion):
    """A CFAR detector over rows of nbins bins on one GPU: `train` training and `guard` guard cells on either side, a
    threshold in dB above the estimated floor, mode ca | go | so; detected runs shorter than min_width are dropped, gaps of at
    most max_gap bins are bridged.  It holds int64 hits[nbins] and the first `capacity` emission records in ascending
    (row, bin_lo) order.  The integer rule is stated in include/ksa_detect.h."""
    _binding, _info_fields = _bind, ("threads", "lds_bytes", "vgprs", "grid", "vec", "rows_per_wg")

    def __init__(self, nbins, train, guard, threshold_db, mode="ca", min_width=1, max_gap=0, capacity=4096, device=0,
                 stream=None):
        self.nbins, self.capacity, self.device = int(nbins), int(capacity), int(device)
        self.params = (int(train), int(guard), float(threshold_db), _mode(mode), int(min_width), int(max_gap))
        self._create(self.device, self.nbins, *self.params, self.capacity, stream=stream)

    # -- detection --------------------------------------------------------------------------------
    def detect_rows_dev(self, rows, nrows=None, row_stride=None, row_count=None, floor=None):
        """nrows float32 rows from device memory (a torch tensor, DevArray pointer or int address), row i at
        rows + i*row_stride floats; asynchronous on the object's stream.  nrows defaults to the first dimension of a 2-D
        tensor.  row_count: device int32 [nrows] that receives every row's emissions; floor: device float32 [nrows][nbins] that
        receives the pooled floor estimate of every bin."""
        if nrows is None:
            shape = getattr(rows, "shape", None)
            if shape is None or len(shape) != 2:
                raise KsaError("detect_rows_dev needs nrows unless rows is a 2-D tensor")
            nrows = shape[0]
        stride = self.nbins if row_stride is None else int(row_stride)
        check(lib().kse_detect_rows_dev(self._h, _ptr(rows), stride, int(nrows), None if row_count is None else _ptr(row_count),
                                        None if floor is None else _ptr(floor)))

    def detect_rows(self, host_rows):
        """float32 [k][nbins] (or one row) from host memory; synchronises."""
        a = np.ascontiguousarray(host_rows, dtype=np.float32)
        if a.size % self.nbins or (a.ndim > 1 and a.shape[-1] != self.nbins):
            raise KsaError("detect_rows wants [k][%d] float32, got %s" % (self.nbins, a.shape))
        if a.size:
            check(lib().kse_detect_rows(self._h, _ptr(a), a.size // self.nbins))

    def set_params(self, train=None, guard=None, threshold_db=None, mode=None, min_width=None, max_gap=None):
        """Replace the detection parameters (None keeps a value); rows already enqueued use the old ones, state is kept."""
        old = self.params
        new = (old[0] if train is None else int(train), old[1] if guard is None else int(guard),
               old[2] if threshold_db is None else float(threshold_db), old[3] if mode is None else _mode(mode),
               old[4] if min_width is None else int(min_width), old[5] if max_gap is None else int(max_gap))
        check(lib().kse_set_params(self._h, *new))
        self.params = new

    def set_row_base(self, row_base):
        """The index the next row gets (and rows_seen)."""
        if not -2 ** 63 <= int(row_base) < 2 ** 63:
            raise KsaError("set_row_base(%d): outside int64" % row_base)
        check(lib().kse_set_row_base(self._h, int(row_base)))

    def merge_hits_dev(self, hits, rows_seen_add=0):
        """hits += another object's hits in device memory (int64 [nbins])."""
        check(lib().kse_merge_hits_dev(self._h, _ptr(hits), int(rows_seen_add)))

    def clear_emissions(self):
        check(lib().kse_clear_emissions(self._h))

    def reset(self):
        check(lib().kse_reset(self._h))

    # -- results ----------------------------------------------------------------------------------
    def hits(self):
        """(int64 [nbins], rows_seen); synchronises."""
        out = np.empty(self.nbins, dtype=np.int64)
        seen = C.c_int64()
        check(lib().kse_read_hits(self._h, _ptr(out), C.byref(seen)))
        return out, seen.value

    @property
    def rows_seen(self):
        seen = C.c_int64()
        check(lib().kse_read_hits(self._h, None, C.byref(seen)))
        return seen.value

    def occupancy(self):
        """float64 [nbins]: the share of the rows seen in which the bin lay inside an emission; 0 when no rows were seen."""
        h, seen = self.hits()
        if seen <= 0:
            return np.zeros(self.nbins, dtype=np.float64)
        return h.astype(np.float64) / seen

    def emissions(self):
        """(structured array of EMISSION_DTYPE: the stored records in ascending (row, bin_lo) order; emissions_total);
        synchronises."""
        stored, total = C.c_int64(), C.c_int64()
        check(lib().kse_read_emissions(self._h, None, 0, C.byref(stored), C.byref(total)))
        out = np.zeros(stored.value, dtype=EMISSION_DTYPE)
        if stored.value:
            check(lib().kse_read_emissions(self._h, _ptr(out), stored.value, C.byref(stored), C.byref(total)))
        return out[:stored.value].copy(), total.value

    def hits_view(self):
        p = C.c_void_p()
        check(lib().kse_hits_dev(self._h, C.byref(p)))
        return DevArray(p.value, (self.nbins,), self, "<i8")
