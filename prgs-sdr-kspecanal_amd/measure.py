"""Band measurements on the GPU: ctypes binding of include/ksa_measure.h (libksa_measure.so, a companion of libksa.so) and the
SpectrumMeter class over it.  A window of a dB row -- the span of an emission record of the signal detector, widened by a
margin, or one of a fixed list of bands -- is measured: integrated (channel) power, the power moments that give centroid and
RMS width, the peak, the occupied bandwidth (the width that holds a share of the power, 99 % by default) and the x-dB width.
The detector's records and their count are read where they lie in device memory.  There is no fallback: a missing library
raises."""
import ctypes as C

import numpy as np

from ._companion import Binding, Companion
from ._lib import KsaError
from .engine import DevArray, _ptr

ABI_VERSION = 1
MAX_NBINS = 1 << 24
MAX_CAPACITY = 1 << 20
MAX_MARGIN = 65536
MAX_BANDS = 1024
WAVE_MAX_BINS = 256
FLAG_MEASURED, FLAG_CLIPPED, FLAG_INVALID = 1, 2, 4

_P = C.c_void_p
_I32, _I64, _F = C.c_int32, C.c_int64, C.c_float

# the 80 bytes of kme_result
RESULT_DTYPE = np.dtype([("row", "<i8"), ("bin_lo", "<i4"), ("bin_hi", "<i4"), ("nvalid", "<i4"), ("flags", "<i4"),
                         ("power", "<f8"), ("m1", "<f8"), ("m2", "<f8"), ("peak_bin", "<i4"), ("peak_db", "<f4"),
                         ("obw_lo", "<i4"), ("obw_hi", "<i4"), ("xdb_lo", "<i4"), ("xdb_hi", "<i4"), ("power_db", "<f4"),
                         ("reserved", "<i4")])
assert RESULT_DTYPE.itemsize == 80
# what a span record begins with (kme_span); detect.EMISSION_DTYPE begins like this
SPAN_HEAD_DTYPE = np.dtype([("row", "<i8"), ("bin_lo", "<i4"), ("bin_hi", "<i4")])

# name -> (restype, argtypes); every symbol include/ksa_measure.h declares
SIGNATURES = {
    "kme_abi_version": (C.c_int, []),
    "kme_last_error": (C.c_char_p, []),
    "kme_create": (C.c_int, [_I32, _I32, _I32, _F, _F, _I32, C.POINTER(_P)]),
    "kme_destroy": (None, [_P]),
    "kme_set_stream": (C.c_int, [_P, _P]),
    "kme_synchronize": (C.c_int, [_P]),
    "kme_set_params": (C.c_int, [_P, _F, _F, _I32]),
    "kme_measure_spans_dev": (C.c_int, [_P, _P, _I64, _I64, _I64, _P, _I64, _P, _I64, _I64]),
    "kme_measure_spans": (C.c_int, [_P, _P, _I64, _I64, _P, _I64, _P, _I64, _I64]),
    "kme_set_bands": (C.c_int, [_P, _P, _I32]),
    "kme_measure_bands_dev": (C.c_int, [_P, _P, _I64, _I64, _I64, _I64]),
    "kme_measure_bands": (C.c_int, [_P, _P, _I64, _I64, _I64]),
    "kme_read_results": (C.c_int, [_P, _P, _I64, _I64]),
    "kme_results_dev": (C.c_int, [_P, C.POINTER(_P)]),
    "kme_reset": (C.c_int, [_P]),
    "kme_kernel_info": (C.c_int, [_P] + [C.POINTER(_I32)] * 6),
}


_bind = Binding("libksa_measure.so", "kme_", ABI_VERSION, SIGNATURES)
LIB_PATH = _bind.path
load, lib, check = _bind.load, _bind.lib, _bind.check


def result_freqs(res, freqs):
    """dict(center_hz, obw_hz, xdb_hz), float64 [len(res)] each, of the result records res from the bin frequencies freqs
    [nbins] (ascending, evenly spaced): the centre is the power centroid bin_lo + m1 / power, the widths count whole bins.
    NaN where a record holds no measurement or no valid bin."""
    r = np.asarray(res)
    f = np.asarray(freqs, dtype=np.float64)
    step = (f[-1] - f[0]) / (len(f) - 1) if len(f) > 1 else 0.0
    ok = ((r["flags"] & FLAG_MEASURED) != 0) & (r["nvalid"] > 0)
    nan = np.full(len(r), np.nan, dtype=np.float64)
    centroid = np.divide(r["m1"], r["power"], out=nan.copy(), where=ok) + r["bin_lo"]
    return {"center_hz": np.where(ok, f[0] + centroid * step, np.nan),
            "obw_hz": np.where(ok, (r["obw_hi"] - r["obw_lo"] + 1) * step, np.nan),
            "xdb_hz": np.where(ok, (r["xdb_hi"] - r["xdb_lo"] + 1) * step, np.nan)}


def acpr(main, adjacent):
    """The adjacent-channel power ratio in dB, float64: 10 log10(power of `adjacent` / power of `main`), record by record
    (either may be one record).  NaN where either holds no measurement or no power."""
    a, b = np.asarray(adjacent), np.asarray(main)
    ok = ((a["flags"] & b["flags"] & FLAG_MEASURED) != 0) & (a["power"] > 0) & (b["power"] > 0)
    out = np.full(np.broadcast(a, b).shape, np.nan, dtype=np.float64)
    ratio = np.divide(a["power"], b["power"], out=np.ones_like(out), where=ok)
    return np.where(ok, 10.0 * np.log10(ratio), out)


class SpectrumMeter(Companion):
    """A meter over rows of nbins bins on one GPU: `occupied` is the share of the power inside the occupied bandwidth, `xdb`
    how far below the peak the x-dB edges lie, `margin` how many bins a span is widened on either side.  It holds `capacity`
    result records; a span's result lies at the span's own index.  The rule is stated in include/ksa_measure.h."""
    _binding, _info_fields = _bind, ("threads", "lds_bytes", "vgprs", "grid", "vec", "form")

    def __init__(self, nbins, capacity=4096, occupied=0.99, xdb=3.0, margin=0, device=0, stream=None):
        self.nbins, self.capacity, self.device = int(nbins), int(capacity), int(device)
        self.params = (float(occupied), float(xdb), int(margin))
        self.bands = np.zeros((0, 2), dtype=np.int32)
        self._create(self.device, self.nbins, self.capacity, *self.params, stream=stream)

    def set_params(self, occupied=None, xdb=None, margin=None):
        """Replace the parameters (None keeps a value); they hold from the next call, results are kept."""
        old = self.params
        new = (old[0] if occupied is None else float(occupied), old[1] if xdb is None else float(xdb),
               old[2] if margin is None else int(margin))
        check(lib().kme_set_params(self._h, *new))
        self.params = new

    def _nrows(self, rows, nrows, what):
        if nrows is not None:
            return int(nrows)
        shape = getattr(rows, "shape", None)
        if shape is None or len(shape) != 2:
            raise KsaError("%s needs nrows unless rows is a 2-D tensor" % what)
        return shape[0]

    def _host_rows(self, host_rows, what):
        a = np.ascontiguousarray(host_rows, dtype=np.float32)
        if a.size % self.nbins or (a.ndim > 1 and a.shape[-1] != self.nbins):
            raise KsaError("%s wants [k][%d] float32, got %s" % (what, self.nbins, a.shape))
        return a

    # -- spans ------------------------------------------------------------------------------------
    def measure_spans_dev(self, rows, spans, total, nrows=None, row_stride=None, row_base=0, span_stride=32,
                          span_capacity=None, first=0):
        """Measure the spans of a list in device memory in nrows float32 rows of device memory, row i at rows + i*row_stride
        floats with the running index row_base + i; asynchronous.  spans: the records, span_stride bytes apart, each beginning
        with int64 row, int32 bin_lo, int32 bin_hi; total: the address of the int64 that counts them, read on the device;
        span_capacity: the records the list has room for (default: this object's capacity).  results[i] is span i's."""
        stride = self.nbins if row_stride is None else int(row_stride)
        cap = self.capacity if span_capacity is None else int(span_capacity)
        check(lib().kme_measure_spans_dev(self._h, _ptr(rows), stride, self._nrows(rows, nrows, "measure_spans_dev"), int(row_base),
                                          _ptr(spans), int(span_stride), _ptr(total), cap, int(first)))

    def measure_spans(self, host_rows, spans, total, row_base=0, span_stride=32, span_capacity=None, first=0):
        """The same over float32 [k][nbins] (or one row) of host memory; the spans stay on the device.  Synchronises."""
        a = self._host_rows(host_rows, "measure_spans")
        cap = self.capacity if span_capacity is None else int(span_capacity)
        if a.size:
            check(lib().kme_measure_spans(self._h, _ptr(a), a.size // self.nbins, int(row_base), _ptr(spans), int(span_stride),
                                          _ptr(total), cap, int(first)))

    @staticmethod
    def detector_list(det):
        """(records address, count address, rows_seen, stored) of a SignalDetector's emission buffer in device memory; the
        detector's stream is synchronised (the two objects may work on different streams)."""
        rec, tot = C.c_void_p(), C.c_void_p()
        stored = C.c_int64()
        det._binding.check(det._binding.lib().kse_emissions_dev(det._h, C.byref(rec), C.byref(tot)))
        det._binding.check(det._binding.lib().kse_read_emissions(det._h, None, 0, C.byref(stored), None))
        return rec.value, tot.value, det.rows_seen, stored.value

    def measure_detector(self, det, rows, row_base, first=0, nrows=None, row_stride=None):
        """Measure a SignalDetector's emissions from index `first` on in the rows they were detected in: rows is host memory
        (numpy, synchronises) or device memory (a tensor, DevArray or address with nrows; asynchronous), row_base the running
        index of its first row.  Result i pairs with emission i; nothing of the list is copied to the host."""
        rec, tot, _, _ = self.detector_list(det)
        if isinstance(rows, np.ndarray):
            self.measure_spans(rows, rec, tot, row_base=row_base, span_stride=32, span_capacity=det.capacity, first=first)
        else:
            self.measure_spans_dev(rows, rec, tot, nrows=nrows, row_stride=row_stride, row_base=row_base, span_stride=32,
                                   span_capacity=det.capacity, first=first)

    # -- bands ------------------------------------------------------------------------------------
    def set_bands(self, bands):
        """The fixed bands: int [nb][2], first and last bin (inclusive) of each, nb 0 .. 1024; synchronises."""
        b = np.ascontiguousarray(bands, dtype=np.int32).reshape(-1, 2)
        check(lib().kme_set_bands(self._h, _ptr(b) if len(b) else None, len(b)))
        self.bands = b.copy()

    def measure_bands_dev(self, rows, nrows=None, row_stride=None, row_base=0, first_slot=0):
        """results[first_slot + r*nb + j] = band j in row r of device memory; asynchronous."""
        stride = self.nbins if row_stride is None else int(row_stride)
        check(lib().kme_measure_bands_dev(self._h, _ptr(rows), stride, self._nrows(rows, nrows, "measure_bands_dev"), int(row_base),
                                          int(first_slot)))

    def measure_bands(self, host_rows, row_base=0, first_slot=0):
        """The same over float32 [k][nbins] (or one row) of host memory; synchronises."""
        a = self._host_rows(host_rows, "measure_bands")
        if a.size:
            check(lib().kme_measure_bands(self._h, _ptr(a), a.size // self.nbins, int(row_base), int(first_slot)))

    # -- results ----------------------------------------------------------------------------------
    def results(self, first=0, count=None):
        """Structured array of RESULT_DTYPE: slots first .. first + count (default: to the end); synchronises."""
        n = self.capacity - int(first) if count is None else int(count)
        out = np.zeros(max(n, 0), dtype=RESULT_DTYPE)
        check(lib().kme_read_results(self._h, _ptr(out) if len(out) else None, int(first), n))
        return out

    def results_view(self):
        """The record buffer as raw bytes [capacity][80] in device memory, for torch.as_tensor."""
        p = C.c_void_p()
        check(lib().kme_results_dev(self._h, C.byref(p)))
        return DevArray(p.value, (self.capacity, RESULT_DTYPE.itemsize), self, "|u1")

    def reset(self):
        check(lib().kme_reset(self._h))
