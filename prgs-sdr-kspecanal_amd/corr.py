"""Matched-filter correlator and peak list on the GPU: ctypes binding of include/ksa_corr.h (libksa_corr.so, a companion of
libksa.so) and the Correlator class over it.  Q templates of K complex samples (a sync word, a preamble, a chirp, a bank of
frequency-offset hypotheses) slide over raw IQ in device memory; every lag gets its correlation r and its normalised metric rho
in [0, 1], and the lags at which rho peaks above a threshold are listed with what a time of arrival and a carrier phase need.
There is no fallback: a missing library raises."""
import ctypes as C

import numpy as np

from ._companion import FORMATS, SAMPLE_DTYPES, Binding, Companion, format_of
from ._lib import KsaError, FMT_C64, FMT_U8, FMT_S8, FMT_S16
from .engine import DevArray, _ptr

ABI_VERSION = 1
MAX_K, MAX_Q, MAX_TEMPLATE_VALUES, MAX_GUARD, MAX_CAPACITY, MAX_IN, MAX_POSITION = 4096, 8, 16384, 4096, 1 << 20, 2 ** 28 - 1, 2 ** 52

_P = C.c_void_p
_I32, _I64, _F = C.c_int32, C.c_int64, C.c_float

# the 36 bytes of kcr_event, no padding
EVENT_DTYPE = np.dtype([("pos", "<i8"), ("block", "<i4"), ("templ", "<i4"), ("metric", "<f4"), ("metric_prev", "<f4"),
                        ("metric_next", "<f4"), ("re", "<f4"), ("im", "<f4")])
assert EVENT_DTYPE.itemsize == 36

# name -> (restype, argtypes); every symbol include/ksa_corr.h declares
SIGNATURES = {
    "kcr_abi_version": (C.c_int, []),
    "kcr_last_error": (C.c_char_p, []),
    "kcr_create": (C.c_int, [_I32, _I32, _F, _F, _I32, _I32, _P, _F, _F, _I32, _I32, _I64, C.POINTER(_P)]),
    "kcr_destroy": (None, [_P]),
    "kcr_set_stream": (C.c_int, [_P, _P]),
    "kcr_synchronize": (C.c_int, [_P]),
    "kcr_out_count": (C.c_int, [_P, _I64, C.POINTER(_I64)]),
    "kcr_process_dev": (C.c_int, [_P, _P, _I64, _P, _P, _I64, C.POINTER(_I64)]),
    "kcr_process": (C.c_int, [_P, _P, _I64, _P, _P, _I64, C.POINTER(_I64)]),
    "kcr_flush": (C.c_int, [_P]),
    "kcr_blocks_dev": (C.c_int, [_P, _P, _I64, _I64, _I64, _P, _P, _I64]),
    "kcr_set_params": (C.c_int, [_P, _F, _F]),
    "kcr_set_templates": (C.c_int, [_P, _P]),
    "kcr_reset": (C.c_int, [_P]),
    "kcr_state": (C.c_int, [_P, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(_I64)]),
    "kcr_read_events": (C.c_int, [_P, _P, _I64, C.POINTER(_I64), C.POINTER(_I64)]),
    "kcr_events_dev": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P)]),
    "kcr_clear_events": (C.c_int, [_P]),
    "kcr_kernel_info": (C.c_int, [_P] + [C.POINTER(_I32)] * 5),
}


_bind = Binding("libksa_corr.so", "kcr_", ABI_VERSION, SIGNATURES)
LIB_PATH = _bind.path
load, lib, check = _bind.load, _bind.lib, _bind.check


def _templates(templates):
    """complex64 [Q][K] from [K] or [Q][K]."""
    t = np.asarray(templates)
    if t.ndim == 1:
        t = t[None, :]
    if t.ndim != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise KsaError("templates want complex [K] or [Q][K], got shape %s" % (t.shape,))
    return np.ascontiguousarray(t, dtype=np.complex64)


def frequency_bank(template, offsets_cycles_per_sample):
    """complex64 [Q][K]: the template shifted by each offset f (cycles per sample), c[k] * exp(2j pi f k), formed in float64:
    a bank of frequency-offset hypotheses for one Correlator."""
    t = np.asarray(template, dtype=np.complex128).reshape(-1)
    f = np.atleast_1d(np.asarray(offsets_cycles_per_sample, dtype=np.float64)).reshape(-1)
    if t.size < 1 or f.size < 1 or not np.all(np.isfinite(f)):
        raise KsaError("frequency_bank wants a template of K >= 1 samples and at least one finite offset")
    k = np.arange(t.size, dtype=np.float64)
    return (t[None, :] * np.exp(2j * np.pi * f[:, None] * k[None, :])).astype(np.complex64)


def refine(events):
    """float64 [len(events)]: the fractional position of every event by the parabola through (pos-1, metric_prev),
    (pos, metric), (pos+1, metric_next); `pos` itself where the parabola is degenerate (no downward curvature)."""
    ev = np.asarray(events)
    pos = ev["pos"].astype(np.float64)
    a, b, c = (ev[k].astype(np.float64) for k in ("metric_prev", "metric", "metric_next"))
    den = a - 2 * b + c
    ok = (den < 0) & np.isfinite(den)
    d = np.zeros_like(pos)
    d[ok] = 0.5 * (a[ok] - c[ok]) / den[ok]
    return pos + np.clip(d, -0.5, 0.5)              # a peak's vertex lies within half a lag; the clip only absorbs rounding


class Correlator(Companion):
    """A matched-filter correlator for Q templates of K samples on one GPU; the contract is include/ksa_corr.h.  templates:
    complex [K] or [Q][K].  fmt: c64 | u8 | s8 | s16 (or the number).  guard None = K.  It holds the first `capacity` events in
    ascending (block, pos, templ) order."""
    _binding, _info_fields = _bind, ("threads", "lds_bytes", "vgprs", "grid", "tile_out")

    def __init__(self, templates, threshold=0.5, min_energy=0.0, guard=None, capacity=4096, max_in=1 << 20, fmt="c64",
                 u8_offset=127.5, u8_scale=127.5, device=0, stream=None):
        self.fmt = format_of(fmt)
        self.templates = _templates(templates)
        self.Q, self.K = (int(v) for v in self.templates.shape)
        self.guard = self.K if guard is None else int(guard)
        self.threshold, self.min_energy = float(threshold), float(min_energy)
        self.capacity, self.max_in, self.device = int(capacity), int(max_in), int(device)
        self.in_dtype = SAMPLE_DTYPES.get(self.fmt, np.dtype(np.complex64))
        self._create(self.device, self.fmt, float(u8_offset), float(u8_scale), self.K, self.Q, _ptr(self.templates),
                     self.threshold, self.min_energy, self.guard, self.capacity, self.max_in, stream=stream)

    # -- the stream form ----------------------------------------------------------------------------
    def out_count(self, n_in):
        n = C.c_int64()
        check(lib().kcr_out_count(self._h, int(n_in), C.byref(n)))
        return n.value

    def process_dev(self, iq, n_in, metric=None, corr=None, out_stride=0):
        """The stream's next n_in samples from device memory; asynchronous.  metric: device float32, corr: device complex64,
        template q's lags at q * out_stride; either may be None.  Returns the number of lags the call completed."""
        n = C.c_int64()
        check(lib().kcr_process_dev(self._h, _ptr(iq), int(n_in), _ptr(metric), _ptr(corr), int(out_stride), C.byref(n)))
        return n.value

    def process(self, samples):
        """The stream's next samples from host memory (complex64 [n], or [n][2] of the integer formats); synchronises.
        Returns (rho float32 [Q][lags], r complex64 [Q][lags])."""
        a = np.ascontiguousarray(samples, dtype=self.in_dtype)
        n_in = a.size if self.fmt == FMT_C64 else a.size // 2
        lags = self.out_count(n_in)
        rho = np.zeros((self.Q, lags), dtype=np.float32)
        r = np.zeros((self.Q, lags), dtype=np.complex64)
        n = C.c_int64()
        check(lib().kcr_process(self._h, _ptr(a), n_in, _ptr(rho), _ptr(r), lags, C.byref(n)))
        return rho, r

    def flush(self):
        """Decide the lags still pending at the end of the stream; stream calls are refused afterwards until reset()."""
        check(lib().kcr_flush(self._h))

    # -- the block form -----------------------------------------------------------------------------
    def blocks_dev(self, iq, nblocks, block_len, block_stride=None, metric=None, corr=None, out_stride=None):
        """nblocks independent blocks of block_len samples, block b at iq + b*block_stride samples (device memory);
        asynchronous.  Dense rows at (b * Q + q) * out_stride.  Returns the lags per block, block_len - K + 1."""
        lags = int(block_len) - self.K + 1
        stride = int(block_len) if block_stride is None else int(block_stride)
        check(lib().kcr_blocks_dev(self._h, _ptr(iq), stride, int(nblocks), int(block_len), _ptr(metric), _ptr(corr),
                                   max(lags, 0) if out_stride is None else int(out_stride)))
        return lags

    # -- state --------------------------------------------------------------------------------------
    def set_params(self, threshold=None, min_energy=None):
        """Replace threshold and min_energy (None keeps a value); they hold from the next call."""
        thr = self.threshold if threshold is None else float(threshold)
        me = self.min_energy if min_energy is None else float(min_energy)
        check(lib().kcr_set_params(self._h, thr, me))
        self.threshold, self.min_energy = thr, me

    def set_templates(self, templates):
        """Replace the templates (the same Q and K); stream state and events are kept.  Synchronises."""
        t = _templates(templates)
        if t.shape != self.templates.shape:
            raise KsaError("set_templates wants %s complex64, got %s" % (self.templates.shape, t.shape))
        check(lib().kcr_set_templates(self._h, _ptr(t)))
        self.templates = t

    def reset(self):
        check(lib().kcr_reset(self._h))

    def state(self):
        """dict(samples_in, lags_done, lags_decided) of the stream."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        check(lib().kcr_state(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"samples_in": a.value, "lags_done": b.value, "lags_decided": c.value}

    # -- results ------------------------------------------------------------------------------------
    def events(self):
        """(structured array of EVENT_DTYPE: the stored records in ascending (block, pos, templ) order; events_total);
        synchronises."""
        stored, total = C.c_int64(), C.c_int64()
        check(lib().kcr_read_events(self._h, None, 0, C.byref(stored), C.byref(total)))
        out = np.zeros(stored.value, dtype=EVENT_DTYPE)
        if stored.value:
            check(lib().kcr_read_events(self._h, _ptr(out), stored.value, C.byref(stored), C.byref(total)))
        return out[:stored.value].copy(), total.value

    def clear_events(self):
        check(lib().kcr_clear_events(self._h))

    def events_view(self):
        """The event buffer as raw bytes [capacity][36] in device memory, for torch.as_tensor."""
        p = C.c_void_p()
        check(lib().kcr_events_dev(self._h, C.byref(p), None))
        return DevArray(p.value, (self.capacity, EVENT_DTYPE.itemsize), self, "|u1")
