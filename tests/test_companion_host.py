"""The layer the six companion libraries share (no GPU needed): csrc_shared/ and _companion.py.  Each library keeps its own
thread-local error string although all six are loaded into one process, nothing of the shared header is exported, every
companion product depends on csrc_shared/ and libksa.so does not, the shared code is defined once, and the six bindings expose
what they exposed before the layer existed."""
import ctypes as C
import importlib
import os
import re
import subprocess
import threading

import numpy as np
import pytest

from conftest import ROOT, load_pkg

PKG_DIR = os.path.join(ROOT, "prgs-sdr-kspecanal_amd")
SHARED = [os.path.join(PKG_DIR, "csrc_shared", f) for f in ("ksa_host.hpp", "ksa_iq.hpp")]

_P = C.c_void_p
_I32, _I64, _U64, _F = C.c_int32, C.c_int64, C.c_uint64, C.c_float

# module -> (file name, symbol prefix, ABI version, SIGNATURES), written out as the bindings stood before they shared _companion.py
SURFACE = {
    "density": ("libksa_density.so", "ksd_", 1, {
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
    }),
    "mask": ("libksa_mask.so", "ksm_", 1, {
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
    }),
    "ddc": ("libksa_ddc.so", "kdc_", 1, {
        "kdc_abi_version": (C.c_int, []),
        "kdc_last_error": (C.c_char_p, []),
        "kdc_create": (C.c_int, [_I32, _I32, _F, _F, _I32, _I32, _P, _U64, _I64, C.POINTER(_P)]),
        "kdc_destroy": (None, [_P]),
        "kdc_set_stream": (C.c_int, [_P, _P]),
        "kdc_synchronize": (C.c_int, [_P]),
        "kdc_out_count": (C.c_int, [_P, _I64, C.POINTER(_I64)]),
        "kdc_process_dev": (C.c_int, [_P, _P, _I64, _P, _I64, C.POINTER(_I64)]),
        "kdc_process": (C.c_int, [_P, _P, _I64, _P, _I64, C.POINTER(_I64)]),
        "kdc_blocks_dev": (C.c_int, [_P, _P, _I64, _I64, _I64, _P, _I64]),
        "kdc_set_tuning": (C.c_int, [_P, _U64]),
        "kdc_set_taps": (C.c_int, [_P, _P]),
        "kdc_reset": (C.c_int, [_P]),
        "kdc_state": (C.c_int, [_P, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(_U64)]),
        "kdc_out_dev": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_I64)]),
        "kdc_kernel_info": (C.c_int, [_P] + [C.POINTER(_I32)] * 6),
    }),
    "detect": ("libksa_detect.so", "kse_", 1, {
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
    }),
    "demod": ("libksa_demod.so", "kdm_", 1, {
        "kdm_abi_version": (C.c_int, []),
        "kdm_last_error": (C.c_char_p, []),
        "kdm_create": (C.c_int, [_I32, _I32, _I32, _I32, _P, _I32, _F, _I64, C.POINTER(_P)]),
        "kdm_destroy": (None, [_P]),
        "kdm_set_stream": (C.c_int, [_P, _P]),
        "kdm_synchronize": (C.c_int, [_P]),
        "kdm_out_count": (C.c_int, [_P, _I64, C.POINTER(_I64)]),
        "kdm_process_dev": (C.c_int, [_P, _P, _I64, _P, _I64, C.POINTER(_I64)]),
        "kdm_process": (C.c_int, [_P, _P, _I64, _P, _I64, C.POINTER(_I64)]),
        "kdm_blocks_dev": (C.c_int, [_P, _P, _I64, _I64, _I64, _P, _I64]),
        "kdm_set_taps": (C.c_int, [_P, _P]),
        "kdm_reset": (C.c_int, [_P]),
        "kdm_state": (C.c_int, [_P, C.POINTER(_I64), C.POINTER(_I64)]),
        "kdm_out_dev": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_I64)]),
        "kdm_read_out": (C.c_int, [_P, _P, _I64, _I64]),
        "kdm_kernel_info": (C.c_int, [_P] + [C.POINTER(_I32)] * 5),
    }),
    "chan": ("libksa_chan.so", "kch_", 1, {
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
    }),
}


@pytest.fixture(scope="module")
def mods():
    load_pkg()
    return {m: importlib.import_module("prgs-sdr-kspecanal_amd." + m) for m in SURFACE}


def _refusals():
    """module -> (call of k??_create that is refused before any device is touched, a text of that refusal no other library has)"""
    taps = np.ones(8, dtype=np.float32)
    p = taps.ctypes.data_as(C.c_void_p)
    return taps, {
        "density": (lambda lib, h: lib.ksd_create(0, 1024, 0, 256, -140.0, 0.0, h), "width 0 must be >= 1"),
        "mask": (lambda lib, h: lib.ksm_create(0, 1024, None, None, 0, 16, h), "min_bins 0 must be >= 1"),
        "ddc": (lambda lib, h: lib.kdc_create(0, 0, 0.0, 1.0, 0, 8, p, 0, 64, h), "decim 0 outside 1..1024"),
        "detect": (lambda lib, h: lib.kse_create(0, 1024, 0, 2, 10.0, 0, 1, 0, 16, h), "train 0 outside 1..1024"),
        "demod": (lambda lib, h: lib.kdm_create(0, 7, 4, 8, p, 0, 1.0, 64, h), "unknown mode 7"),
        "chan": (lambda lib, h: lib.kch_create(0, 0, 0.0, 1.0, 3, 1, 8, p, 64, h), "nchan 3 must be a power of two, 2..1024"),
    }


def _last_errors(mods):
    return {m: getattr(mods[m].lib(), SURFACE[m][1] + "last_error")().decode() for m in SURFACE}


def test_every_library_keeps_its_own_thread_local_error_string(mods):
    taps, refusals = _refusals()
    for m, (create, text) in refusals.items():
        h = C.c_void_p(1)
        assert create(mods[m].lib(), C.byref(h)) != 0 and h.value is None, m
        assert _last_errors(mods)[m] == text, m
    # all six have failed by now, each after its predecessors: none has overwritten another's text
    assert _last_errors(mods) == {m: text for m, (_, text) in refusals.items()}
    seen = {}
    t = threading.Thread(target=lambda: seen.update(_last_errors(mods)))
    t.start()
    t.join()
    assert seen == {m: "" for m in SURFACE}, seen
    assert _last_errors(mods) == {m: text for m, (_, text) in refusals.items()}
    # check() raises the library's own text
    for m, (create, text) in refusals.items():
        with pytest.raises(mods[m].KsaError, match=re.escape(text)):
            mods[m].check(create(mods[m].lib(), C.byref(C.c_void_p())))


def test_nothing_of_the_shared_header_is_exported():
    for m, (file_name, prefix, _, signatures) in SURFACE.items():
        nm = subprocess.run(["nm", "-D", "--defined-only", "-C", os.path.join(PKG_DIR, file_name)], capture_output=True, text=True)
        assert nm.returncode == 0, nm.stderr
        defined = [ln.split(None, 2) for ln in nm.stdout.splitlines()]
        defined = [(f[1], f[2]) for f in defined if len(f) == 3]
        leaked = [(t, name) for t, name in defined if t in "TWVBD"
                  and any(w in name for w in ("fail", "g_err", "DeviceGuard", "check_taps", "ceil_div"))]
        assert not leaked, (file_name, leaked)
        assert {name for t, name in defined if t == "T" and name.startswith(prefix)} == set(signatures), file_name


def test_companions_depend_on_the_shared_directory_and_libksa_does_not(mods):
    build = importlib.import_module("prgs-sdr-kspecanal_amd.build")
    for file_name, _, _, _ in SURFACE.values():
        deps = {os.path.realpath(f) for f in build.JOBS[os.path.join(build.HERE, file_name)][2]()}
        assert {os.path.realpath(f) for f in SHARED} <= deps, file_name
    for out in (build.OUT, build.OUT_EXP):
        deps = {os.path.realpath(f) for f in build.JOBS[out][2]()}
        assert not deps & {os.path.realpath(f) for f in SHARED}, out
        assert not [f for f in deps if "csrc_shared" in f], out
    assert len(build.JOBS) == 8 and build.sources() == build.JOBS[build.OUT][2]()


def _files_with(pattern, top=PKG_DIR, suffixes=(".py", ".hip", ".hpp", ".inc", ".h")):
    hits = []
    for d, dirs, files in os.walk(top):
        dirs[:] = [x for x in dirs if x != "__pycache__"]
        for f in files:
            if f.endswith(suffixes) and re.search(pattern, open(os.path.join(d, f), errors="replace").read()):
                hits.append(os.path.relpath(os.path.join(d, f), PKG_DIR))
    return sorted(hits)


def test_the_shared_code_is_defined_once():
    assert _files_with(r"struct DeviceGuard") == ["csrc/ksa_api.hip", "csrc_shared/ksa_host.hpp"]
    assert [f for f in _files_with(r"float2 unpack_s16\(") if not f.startswith("csrc/")] == ["csrc_shared/ksa_iq.hpp"]
    assert _files_with(r"def load\(") == ["_companion.py", "_lib.py"]
    assert _files_with(r"thread_local std::string g_err") == ["csrc/ksa_api.hip", "csrc_shared/ksa_host.hpp"]
    assert not [f for f in _files_with(r"__cuda_array_interface__") if f != "engine.py"]


def test_the_binding_surface_is_what_it_was(mods):
    for m, (file_name, prefix, abi, signatures) in SURFACE.items():
        X = mods[m]
        assert X.SIGNATURES == signatures, m
        assert X.ABI_VERSION == abi and os.path.basename(X.LIB_PATH) == file_name, m
        assert os.path.dirname(X.LIB_PATH) == PKG_DIR, m
        assert callable(X.load) and callable(X.lib) and callable(X.check), m
        assert issubclass(X.KsaError, RuntimeError) and X.KsaError is load_pkg().KsaError, m
        assert X.lib() is X.lib() and getattr(X.lib(), prefix + "abi_version")() == abi, m
        missing = os.path.join(PKG_DIR, "no_such_" + file_name)
        with pytest.raises(X.KsaError) as e:
            X.load(missing)
        assert str(e.value) == ("%s is missing at %s -- build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950); "
                                "there is no CPU fallback" % (file_name, missing)), m
    ddc, demod, engine = mods["ddc"], mods["demod"], importlib.import_module("prgs-sdr-kspecanal_amd.engine")
    assert ddc.DevArray is engine.DevArray and demod.DevArray is engine.DevArray
    v = engine.DevArray(4096, (2, 3), None, "<i8").__cuda_array_interface__
    assert (v["typestr"], v["shape"], v["data"]) == ("<i8", (2, 3), (4096, False))
    assert engine.DevArray(4096, (5,), None).__cuda_array_interface__["typestr"] == "<f4"
