"""Emission linker and track list on the GPU: ctypes binding of include/ksa_track.h (libksa_track.so, a companion of libksa.so)
and the EmissionTracker class over it.  The per-row emissions of a SignalDetector (row, bin_lo, bin_hi, peak, floor) are joined
into time-frequency tracks -- connected components of "overlaps within bin_slop bins, at most row_gap rows apart" -- and every
track is listed with its first and last row, its band, its peak and what its drift is read from.  Every decision is an integer.
There is no fallback: a missing library raises."""
import ctypes as C

import numpy as np

from ._companion import Binding, Companion
from ._lib import KsaError
from .engine import DevArray, _ptr

ABI_VERSION = 1
MAX_NBINS, MAX_SPANS, MAX_ROW_GAP, MAX_CAPACITY = 1 << 24, 1 << 22, 1024, 1 << 20
FLAG_OPEN_END = 1

_P = C.c_void_p
_I32, _I64 = C.c_int32, C.c_int64

# the 32 bytes of ktr_span: byte for byte detect.EMISSION_DTYPE
SPAN_DTYPE = np.dtype([("row", "<i8"), ("bin_lo", "<i4"), ("bin_hi", "<i4"), ("peak_bin", "<i4"), ("ndet", "<i4"),
                       ("peak_db", "<f4"), ("floor_db", "<f4")])
# the 80 bytes of ktr_track, no padding
TRACK_DTYPE = np.dtype([("row_first", "<i8"), ("row_last", "<i8"), ("peak_row", "<i8"), ("cells", "<i8"), ("sum_mid2", "<i8"),
                        ("bin_lo", "<i4"), ("bin_hi", "<i4"), ("nspans", "<i4"), ("peak_bin", "<i4"), ("mid2_first", "<i4"),
                        ("mid2_last", "<i4"), ("first_span", "<i4"), ("flags", "<i4"), ("peak_db", "<f4"), ("floor_db", "<f4")])
TRACK_OFFSETS = {"row_first": 0, "row_last": 8, "peak_row": 16, "cells": 24, "sum_mid2": 32, "bin_lo": 40, "bin_hi": 44,
                 "nspans": 48, "peak_bin": 52, "mid2_first": 56, "mid2_last": 60, "first_span": 64, "flags": 68, "peak_db": 72,
                 "floor_db": 76}
assert SPAN_DTYPE.itemsize == 32 and TRACK_DTYPE.itemsize == 80
assert {n: TRACK_DTYPE.fields[n][1] for n in TRACK_DTYPE.names} == TRACK_OFFSETS

# name -> (restype, argtypes); every symbol include/ksa_track.h declares
SIGNATURES = {
    "ktr_abi_version": (C.c_int, []),
    "ktr_last_error": (C.c_char_p, []),
    "ktr_create": (C.c_int, [_I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, C.POINTER(_P)]),
    "ktr_destroy": (None, [_P]),
    "ktr_set_stream": (C.c_int, [_P, _P]),
    "ktr_synchronize": (C.c_int, [_P]),
    "ktr_set_params": (C.c_int, [_P, _I32, _I32, _I32, _I32]),
    "ktr_link_dev": (C.c_int, [_P, _P, _I64, _P, _I64, _P]),
    "ktr_link": (C.c_int, [_P, _P, _I64, _I64, _P]),
    "ktr_read_tracks": (C.c_int, [_P, _P, _I64] + [C.POINTER(_I64)] * 4),
    "ktr_read_labels": (C.c_int, [_P, _P, _I64, C.POINTER(_I64)]),
    "ktr_tracks_dev": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P)]),
    "ktr_clear": (C.c_int, [_P]),
    "ktr_kernel_info": (C.c_int, [_P] + [C.POINTER(_I32)] * 5),
}


_bind = Binding("libksa_track.so", "ktr_", ABI_VERSION, SIGNATURES)
LIB_PATH = _bind.path
load, lib, check = _bind.load, _bind.lib, _bind.check


def track_times_freqs(tracks, freqs, row_period_s):
    """What a track list says in units: dict of float64 arrays [len(tracks)] from the bin frequencies freqs [nbins] (ascending,
    evenly spaced) and the time between two rows: t_start_s = row_first * row_period_s, duration_s = (row_last - row_first + 1)
    * row_period_s, center_hz = the middle between the lowest and the highest bin, width_hz counting whole bins, and
    drift_hz_per_s = the movement of the span centre from the first member to the last, (mid2_last - mid2_first) / 2 bins over
    row_last - row_first rows; 0 for a track of one row."""
    tr = np.asarray(tracks)
    f = np.asarray(freqs, dtype=np.float64)
    step = (f[-1] - f[0]) / (len(f) - 1) if len(f) > 1 else 0.0
    period = float(row_period_s)
    rows = (tr["row_last"] - tr["row_first"]).astype(np.float64)
    moved = (tr["mid2_last"].astype(np.float64) - tr["mid2_first"].astype(np.float64)) / 2 * step
    drift = np.zeros(len(tr), dtype=np.float64)
    if period > 0:
        np.divide(moved, rows * period, out=drift, where=rows > 0)
    return {"t_start_s": tr["row_first"].astype(np.float64) * period, "duration_s": (rows + 1) * period,
            "center_hz": (f[tr["bin_lo"]] + f[tr["bin_hi"]]) / 2,
            "width_hz": (tr["bin_hi"] - tr["bin_lo"] + 1).astype(np.float64) * step, "drift_hz_per_s": drift}


class EmissionTracker(Companion):
    """A linker of emission records on one GPU; the contract is include/ksa_track.h.  Spans at most row_gap missing rows apart
    whose bins overlap or miss each other by at most bin_slop are joined; components spanning fewer than min_rows rows or
    holding fewer than min_spans spans are dropped.  It holds the first `capacity` tracks of the last link in ascending
    first_span order; every link replaces the result of the one before."""
    _binding, _info_fields = _bind, ("threads", "lds_bytes", "vgprs", "grid", "launches")

    def __init__(self, nbins, row_gap=0, bin_slop=0, min_rows=1, min_spans=1, capacity=4096, max_spans=1 << 20, device=0,
                 stream=None):
        self.nbins, self.capacity, self.max_spans, self.device = int(nbins), int(capacity), int(max_spans), int(device)
        self.params = (int(row_gap), int(bin_slop), int(min_rows), int(min_spans))
        self._create(self.device, self.nbins, self.max_spans, *self.params, self.capacity, stream=stream)

    def set_params(self, row_gap=None, bin_slop=None, min_rows=None, min_spans=None):
        """Replace the linking parameters (None keeps a value); they hold from the next link."""
        new = tuple(o if v is None else int(v) for o, v in zip(self.params, (row_gap, bin_slop, min_rows, min_spans)))
        check(lib().ktr_set_params(self._h, *new))
        self.params = new

    # -- linking ----------------------------------------------------------------------------------
    def link(self, spans, row_end):
        """Link the records `spans` (SPAN_DTYPE, or detect.EMISSION_DTYPE: the same bytes) from host memory; a list that
        breaks the order or the ranges raises KsaError naming the first offending index.  Synchronises; returns the labels,
        int32 [len(spans)]."""
        a = np.ascontiguousarray(spans)
        if a.dtype.itemsize != SPAN_DTYPE.itemsize or a.dtype.names != SPAN_DTYPE.names:
            raise KsaError("link wants records of SPAN_DTYPE (32 bytes), got %s" % (a.dtype,))
        labels = np.full(a.size, -1, dtype=np.int32)
        check(lib().ktr_link(self._h, _ptr(a) if a.size else None, a.size, int(row_end), _ptr(labels) if a.size else None))
        return labels

    def link_dev(self, spans, n_max, n_dev=None, row_end=0, labels=None):
        """Link n_max records in device memory (a torch tensor, DevArray or int address); asynchronous.  n_dev: the address of
        one int64 in device memory that holds the number of records, clamped to 0 .. n_max on the device, or None for n_max.
        labels: device int32 [n_max], or None.  A list that breaks the rules is only counted: tracks() raises then."""
        check(lib().ktr_link_dev(self._h, _ptr(spans), int(n_max), None if n_dev is None else _ptr(n_dev), int(row_end),
                                 None if labels is None else _ptr(labels)))

    def link_detector(self, det):
        """Link a SignalDetector's emission buffer where it lies: its records and its emissions_total stay on the device, the
        rows it has seen are row_end.  The detector's stream is synchronised first (the two objects may work on different
        streams); the link itself is asynchronous and nothing is copied to the host."""
        if det.capacity > self.max_spans:
            raise KsaError("the detector's buffer holds %d emissions, this tracker links at most max_spans = %d"
                           % (det.capacity, self.max_spans))
        rec, tot = C.c_void_p(), C.c_void_p()
        det._binding.check(det._binding.lib().kse_emissions_dev(det._h, C.byref(rec), C.byref(tot)))
        det.synchronize()
        self.link_dev(rec.value, det.capacity, tot.value, det.rows_seen)

    def clear(self):
        check(lib().ktr_clear(self._h))

    # -- results ----------------------------------------------------------------------------------
    def counts(self):
        """dict(stored, tracks_total, components_total, bad_spans) of the last link; synchronises."""
        v = [C.c_int64() for _ in range(4)]
        check(lib().ktr_read_tracks(self._h, None, 0, *[C.byref(x) for x in v]))
        return dict(zip(("stored", "tracks_total", "components_total", "bad_spans"), [x.value for x in v]))

    def tracks(self):
        """(structured array of TRACK_DTYPE: the stored records in ascending first_span order; tracks_total;
        components_total); synchronises.  Raises KsaError when the linked list broke the rules (bad_spans > 0)."""
        c = self.counts()
        if c["bad_spans"]:
            raise KsaError("%d spans of the linked list are out of range or out of order: nothing was linked" % c["bad_spans"])
        out = np.zeros(c["stored"], dtype=TRACK_DTYPE)
        if c["stored"]:
            check(lib().ktr_read_tracks(self._h, _ptr(out), c["stored"], None, None, None, None))
        return out, c["tracks_total"], c["components_total"]

    def labels(self):
        """int32 [n] of the last link: the rank of every span's track, -1 where its component was filtered out; synchronises."""
        n = C.c_int64()
        check(lib().ktr_read_labels(self._h, None, 0, C.byref(n)))
        out = np.full(n.value, -1, dtype=np.int32)
        if n.value:
            check(lib().ktr_read_labels(self._h, _ptr(out), n.value, None))
        return out

    def tracks_view(self):
        """The record buffer as raw bytes [capacity][80] in device memory, for torch.as_tensor."""
        p = C.c_void_p()
        check(lib().ktr_tracks_dev(self._h, C.byref(p), None))
        return DevArray(p.value, (self.capacity, TRACK_DTYPE.itemsize), self, "|u1")

    def counters_view(self):
        """int64 [4] in device memory: tracks_total, components_total, bad_spans, n."""
        p = C.c_void_p()
        check(lib().ktr_tracks_dev(self._h, None, C.byref(p)))
        return DevArray(p.value, (4,), self, "<i8")
