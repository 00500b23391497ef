"""ksa_create with a raw ksa_config, past every check of SpectrumEngine -- TEST INFRASTRUCTURE beside the contract tests.

create(**fields) fills a valid small config (N = 64, one window at 0, no scan geometry), replaces the named fields and returns
(return code, error text, handle).  REFUSALS lists the configs that include/ksa.h says ksa_create refuses, each with the words
its error text must hold; the bounds are read from the header."""
import ctypes as C
import importlib
import os
import re

import numpy as np

from conftest import ROOT, load_pkg

INT32_MAX = 2 ** 31 - 1
_HDR = open(os.path.join(ROOT, "include", "ksa.h")).read()
MAX_FULL_SIZE = int(re.search(r"#define KSA_MAX_FULL_SIZE (\d+)", _HDR).group(1))
MAX_SCAN_TOTAL = int(re.search(r"#define KSA_MAX_SCAN_TOTAL_ENTRIES (\d+)", _HDR).group(1))
# the bounds, derived again from what they protect: (full_size * 8 bytes) and (3 * total + element) must fit an int32
assert MAX_FULL_SIZE == INT32_MAX // 8 and 4 * MAX_SCAN_TOTAL - 1 == INT32_MAX


def lib_module():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd._lib")


def create(n=64, full_size=None, starts=(0,), taps=None, mag_scale=1.0, cumu_mode=1, u8_scale=127.5, max_frames=4,
           scan_total_entries=0, scan_hop=0, scan_hm_width=0):
    """(return code, error text, handle) of ksa_create on the config these fields describe."""
    _lib = lib_module()
    starts = np.ascontiguousarray(starts, dtype=np.int32)
    win = np.ascontiguousarray(np.ones(n) if taps is None else taps, dtype=np.float32)
    cfg = _lib.Config(abi_version=_lib.lib.ksa_abi_version(), device=0, fft_size=n, full_size=8 * n if full_size is None else full_size,
                      num_windows=len(starts), window_starts=starts.ctypes.data_as(C.POINTER(C.c_int32)),
                      window=win.ctypes.data_as(C.POINTER(C.c_float)), mag_scale=mag_scale, cumu_mode=cumu_mode, gain=0.0, min_amp=0.0,
                      hm_width=16, max_frames=max_frames, u8_offset=127.5, u8_scale=u8_scale,
                      scan_total_entries=scan_total_entries, scan_hop=scan_hop, scan_hm_width=scan_hm_width)
    h = C.c_void_p()
    rc = _lib.lib.ksa_create(C.byref(cfg), C.byref(h))
    return rc, _lib.lib.ksa_last_error().decode(), h


def destroy(h):
    lib_module().lib.ksa_destroy(h)


# (id, fields of create(), words the error text must hold: the field's name and the offending value)
REFUSALS = [
    ("start_int32_max", dict(full_size=512, starts=(0, INT32_MAX, 64)), ("window_starts[1]", str(INT32_MAX))),
    ("start_one_past_the_block", dict(full_size=515, starts=(0, 515 - 64 + 1)), ("window_starts[1]", "452", "515")),
    ("start_negative", dict(full_size=512, starts=(64, 0, -1)), ("window_starts[2]", "-1")),
    ("scan_total_negative", dict(scan_total_entries=-512, scan_hop=32, scan_hm_width=512), ("scan_total_entries", "-512")),
    ("scan_total_past_int_indexing", dict(scan_total_entries=MAX_SCAN_TOTAL + 512, scan_hop=32, scan_hm_width=512),
     ("scan_total_entries", str(MAX_SCAN_TOTAL + 512), str(MAX_SCAN_TOTAL))),
    ("full_size_past_32bit_byte_offsets", dict(full_size=MAX_FULL_SIZE + 1), ("full_size", str(MAX_FULL_SIZE + 1), str(MAX_FULL_SIZE))),
    ("u8_scale_nan", dict(u8_scale=float("nan")), ("u8_scale", "nan")),
    ("u8_scale_inf", dict(u8_scale=float("inf")), ("u8_scale", "inf")),
    ("u8_scale_minus_inf", dict(u8_scale=float("-inf")), ("u8_scale", "-inf")),
]
# the same fields one step inside the bounds are accepted (needs a device: the GPU tests create and destroy them)
ACCEPTED = [
    ("start_last_that_fits", dict(full_size=515, starts=(0, 515 - 64))),
    ("scan_total_small", dict(scan_total_entries=512, scan_hop=32, scan_hm_width=512)),
]


def assert_refused(fields, words):
    """ksa_create must return non-zero, hand back a null handle and name the field.  A config that is wrongly accepted fails on
    the return code; its engine is destroyed and nothing is ever launched on it."""
    rc, err, h = create(**fields)
    if rc == 0:
        destroy(h)
    assert rc != 0, "ksa_create accepted %r" % (fields,)
    assert not h.value, "a refused ksa_create left a handle"
    for w in words:
        assert w in err, "error text %r lacks %r" % (err, w)
