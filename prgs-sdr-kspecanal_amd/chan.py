"""Polyphase channelizer on the GPU: ctypes binding of include/ksa_chan.h (libksa_chan.so, a companion of libksa.so) and the
Channelizer class over it.  One wideband IQ stream becomes all M of its equally spaced channels at once, each at 0 Hz, low-pass
filtered by one prototype and decimated by D = M / O; the result is channel-major complex64 in device memory, which is what
Demodulator.blocks_dev (nblocks = M, block_stride = the channel stride) and the engine's frames_dev already accept.  There is no
fallback: a missing library raises."""
import ctypes as C

import numpy as np

from ._companion import Binding, Companion, host_iq
from ._lib import KsaError, FMT_C64, FMT_U8, FMT_S8, FMT_S16
from .engine import DevArray, _ptr, window_table

ABI_VERSION = 1
MIN_CHAN, MAX_CHAN, MAX_BRANCH_TAPS, MAX_TAPS, MAX_IN = 2, 1024, 32, 8192, 2 ** 28 - 1
FORM_LDS = 0

_P = C.c_void_p
_I32, _I64, _F = C.c_int32, C.c_int64, C.c_float

# name -> (restype, argtypes); every symbol include/ksa_chan.h declares
SIGNATURES = {
    "kch_abi_version": (C.c_int, []),
    "kch_last_error": (C.c_char_p, []),
    "kch_create": (C.c_int, [_I32, _I32, _F, _F, _I32, _I32, _I32, _P, _I64, C.POINTER(_P)]),
    "kch_destroy": (None, [_P]),
    "kch_set_stream": (C.c_int, [_P, _P]),
    "kch_synchronize": (C.c_int, [_P]),
    "kch_out_count": (C.c_int, [_P, _I64, C.POINTER(_I64)]),
    "kch_process_dev": (C.c_int, [_P, _P, _I64, _P, _I64, C.POINTER(_I64)]),
    "kch_process": (C.c_int, [_P, _P, _I64, _P, _I64, C.POINTER(_I64)]),
    "kch_blocks_dev": (C.c_int, [_P, _P, _I64, _I64, _I64, _P, _I64]),
    "kch_channel_power": (C.c_int, [_P, _I64, _I64, _P]),
    "kch_set_taps": (C.c_int, [_P, _P]),
    "kch_reset": (C.c_int, [_P]),
    "kch_state": (C.c_int, [_P, C.POINTER(_I64), C.POINTER(_I64)]),
    "kch_out_dev": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_I64), C.POINTER(_I64), C.POINTER(_I64)]),
    "kch_read_out": (C.c_int, [_P, _P, _I64, _I64, _I64]),
    "kch_kernel_info": (C.c_int, [_P] + [C.POINTER(_I32)] * 6),
}


_bind = Binding("libksa_chan.so", "kch_", ABI_VERSION, SIGNATURES)
LIB_PATH = _bind.path
load, lib, check = _bind.load, _bind.lib, _bind.check


def chan_prototype(nchan, taps_per_branch=8, cutoff=1.0, window="hamming"):
    """float32 [nchan * taps_per_branch]: sinc(cutoff * t / nchan) * window_table(window, T) with t centred, normalised in
    float64 to sum 1 (DC gain 1), symmetric.  cutoff 1.0 puts the -6 dB point at half the channel spacing, fs / (2 nchan), where
    neighbouring channels meet: the choice for oversample 2 and 4, whose output band (2 or 4 channel spacings wide) still holds
    the filter's skirts without aliasing.  At oversample 1 the output band is one channel spacing wide and everything beyond
    +-fs / (2 nchan) folds back, so take cutoff about 0.8 there and leave the channel edges to the transition band."""
    nchan, taps_per_branch = int(nchan), int(taps_per_branch)
    n = nchan * taps_per_branch
    if not (MIN_CHAN <= nchan <= MAX_CHAN and nchan & (nchan - 1) == 0 and 1 <= taps_per_branch <= MAX_BRANCH_TAPS
            and n <= MAX_TAPS and 0 < cutoff <= 2):
        raise KsaError("chan_prototype wants nchan a power of two %d..%d, taps_per_branch 1..%d, nchan * taps_per_branch <= %d "
                       "and 0 < cutoff <= 2" % (MIN_CHAN, MAX_CHAN, MAX_BRANCH_TAPS, MAX_TAPS))
    t = np.arange(n, dtype=np.float64) - (n - 1) / 2
    h = np.sinc(cutoff * t / nchan) * np.asarray(window_table(window, n), dtype=np.float64)
    h = (h + h[::-1]) / 2
    return (h / h.sum()).astype(np.float32)


def channel_freqs(nchan, sampling_rate, center=0.0):
    """float64 [nchan]: the centre frequency of channel c, center + c * fs / nchan for c < nchan / 2 and
    center + (c - nchan) * fs / nchan from nchan / 2 on (the negative frequencies)."""
    c = np.arange(int(nchan))
    return center + np.where(c < nchan // 2, c, c - nchan) * (float(sampling_rate) / nchan)


class Channelizer(Companion):
    """M-channel polyphase filter bank for one IQ stream on one GPU; the contract is include/ksa_chan.h.
    out_stride is the row stride of the STREAM form in the object's own buffer, ceil(max_in / D) + 1, fixed at construction.
    After blocks_dev into the own buffer the rows lie J apart (what blocks_dev returned): layout() and `out` follow the last
    call, out_stride does not."""
    _binding, _info_fields = _bind, ("threads", "lds_bytes", "vgprs", "grid", "tile_cols", "form")

    def __init__(self, fmt, nchan, oversample, taps, max_in=1 << 20, device=0, stream=None, u8_offset=127.5, u8_scale=127.5):
        self.fmt, self.nchan, self.oversample = int(fmt), int(nchan), int(oversample)
        self.device, self.max_in = int(device), int(max_in)
        self.taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        self.ntaps = int(self.taps.size)
        if self.nchan < 1 or self.ntaps < 1 or self.ntaps % self.nchan:
            raise KsaError("Channelizer wants nchan * taps_per_branch taps, got %d taps for %d channels" % (self.ntaps, self.nchan))
        self.taps_per_branch = self.ntaps // self.nchan
        self.decim = max(self.nchan // max(self.oversample, 1), 1)
        self._create(self.device, self.fmt, u8_offset, u8_scale, self.nchan, self.oversample, self.taps_per_branch,
                     _ptr(self.taps), self.max_in, stream=stream)
        self.first = -(-(self.ntaps - 1) // self.decim)
        p, rows, stride, cap = C.c_void_p(), C.c_int64(), C.c_int64(), C.c_int64()
        check(lib().kch_out_dev(self._h, C.byref(p), C.byref(rows), C.byref(stride), C.byref(cap)))
        self._out, self.out_stride, self.out_capacity = p.value, stride.value, cap.value

    # -- the stream form ----------------------------------------------------------------------------
    def out_count(self, n_in):
        n = C.c_int64()
        check(lib().kch_out_count(self._h, int(n_in), C.byref(n)))
        return n.value

    def process_dev(self, iq, n_in, out=None, chan_stride=0):
        """The stream's next n_in samples from device memory; asynchronous.  out: a device complex64 buffer, channel c at
        c * chan_stride, or None for the object's own (self.out, at self.out_stride).  Returns the number of columns."""
        n = C.c_int64()
        check(lib().kch_process_dev(self._h, _ptr(iq), int(n_in), _ptr(out), int(chan_stride), C.byref(n)))
        return n.value

    def process(self, samples):
        """The stream's next samples from host memory (complex64 [n], or [2n] uint8 / int8 / int16 I,Q); complex64
        [nchan][columns]; synchronises."""
        a, n_in = host_iq(samples, self.fmt)
        cols = self.out_count(n_in)
        out = np.empty((self.nchan, cols), dtype=np.complex64)
        n = C.c_int64()
        check(lib().kch_process(self._h, _ptr(a), n_in, _ptr(out), cols, C.byref(n)))
        return out

    # -- the block form -----------------------------------------------------------------------------
    def block_out_count(self, block_len):
        return (int(block_len) - 1) // self.decim - self.first + 1

    def block_len_for(self, columns):
        """The block length that yields exactly `columns` columns per block."""
        return self.decim * (self.first + int(columns) - 1) + 1

    def blocks_dev(self, iq, nblocks, block_len, block_stride=None, out=None, chan_stride=None):
        """nblocks independent captures of block_len samples, block b at iq + b*block_stride samples; asynchronous.  Block b,
        channel c, column j goes to out[(b * nchan + c) * chan_stride + j]; out None: the object's own buffer at stride J.
        Returns J, the columns per block."""
        j = self.block_out_count(block_len)
        stride = int(block_len) if block_stride is None else int(block_stride)
        check(lib().kch_blocks_dev(self._h, _ptr(iq), stride, int(nblocks), int(block_len), _ptr(out),
                                   j if chan_stride is None else int(chan_stride)))
        return j

    # -- read-outs ----------------------------------------------------------------------------------
    def channel_power(self, first, count):
        """float64 [nchan]: per channel the sum of |y|^2 over values [first, first + count) of its rows of the object's own
        buffer; synchronises."""
        p = np.empty(self.nchan, dtype=np.float64)
        check(lib().kch_channel_power(self._h, int(first), int(count), _ptr(p)))
        return p

    def read_out(self, chan, first, count):
        """complex64 [count] of row `chan` of the object's own buffer; synchronises."""
        out = np.empty(int(count), dtype=np.complex64)
        check(lib().kch_read_out(self._h, _ptr(out), int(chan), int(first), int(count)))
        return out

    # -- state --------------------------------------------------------------------------------------
    def set_taps(self, taps):
        """Replace the taps (the same count); the history is kept.  Synchronises."""
        t = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        if t.size != self.ntaps:
            raise KsaError("set_taps wants [%d] float32, got %s" % (self.ntaps, t.shape))
        check(lib().kch_set_taps(self._h, _ptr(t)))
        self.taps = t

    def reset(self):
        check(lib().kch_reset(self._h))

    def state(self):
        """dict(samples_in, samples_out) of the stream."""
        a, b = C.c_int64(), C.c_int64()
        check(lib().kch_state(self._h, C.byref(a), C.byref(b)))
        return {"samples_in": a.value, "samples_out": b.value}

    def layout(self):
        """(rows, row_stride) of what the last call left in the object's own buffer."""
        p, rows, stride = C.c_void_p(), C.c_int64(), C.c_int64()
        check(lib().kch_out_dev(self._h, C.byref(p), C.byref(rows), C.byref(stride), None))
        return rows.value, stride.value

    @property
    def out(self):
        """The object's own buffer as the last call laid it out, complex64 [rows][row_stride] (stream form:
        [nchan][out_stride]), for torch.as_tensor."""
        rows, stride = self.layout()
        return DevArray(self._out, (rows, stride), self, "<c8")

    @property
    def out_ptr(self):
        return self._out
