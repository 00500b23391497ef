"""The layer the companion libraries share (no GPU needed): csrc_shared/, _companion.py and build.py's one table.  Over every
record of companion_helper.COMPANIONS: each library keeps its own thread-local error string although all are loaded into one
process, nothing of the shared header is exported, no library and no binding holds a name of another, every binding exposes the
same surface, the shared code is included and defined once, and the build table is what is written out here."""
import ctypes as C
import importlib
import os
import re
import threading

import pytest

from companion_helper import BY_MODULE, COMPANIONS, PKG_DIR, PREFIXES, SHARED, exported
from conftest import ROOT, load_pkg

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


# product -> (source directory, the .hip that is compiled, public header, extra flags), in the order they are built
PRODUCTS = [
    ("libksa.so", ("csrc", "ksa_api.hip", "ksa.h", [])),
    ("libksa_exp.so", ("csrc", "ksa_api.hip", "ksa.h", ["-DKSA_EXPERIMENTS"])),
    ("libksa_density.so", ("csrc_density", "ksd_api.hip", "ksa_density.h", [])),
    ("libksa_mask.so", ("csrc_mask", "ksm_api.hip", "ksa_mask.h", [])),
    ("libksa_ddc.so", ("csrc_ddc", "kdc_api.hip", "ksa_ddc.h", [])),
    ("libksa_detect.so", ("csrc_detect", "kse_api.hip", "ksa_detect.h", [])),
    ("libksa_demod.so", ("csrc_demod", "kdm_api.hip", "ksa_demod.h", [])),
    ("libksa_chan.so", ("csrc_chan", "kch_api.hip", "ksa_chan.h", [])),
    ("libksa_resamp.so", ("csrc_resamp", "krs_api.hip", "ksa_resamp.h", [])),
    ("libksa_corr.so", ("csrc_corr", "kcr_api.hip", "ksa_corr.h", [])),
    ("libksa_pulse.so", ("csrc_pulse", "kpl_api.hip", "ksa_pulse.h", [])),
    ("libksa_track.so", ("csrc_track", "ktr_api.hip", "ksa_track.h", [])),
    ("libksa_iqfix.so", ("csrc_iqfix", "kqf_api.hip", "ksa_iqfix.h", [])),
]
DELETED_TABLES = ("MORE_PRODUCTS", "LATER_PRODUCTS", "PULSE_PRODUCTS", "TRACK_PRODUCTS", "IQFIX_PRODUCTS", "TABLES", "MORE_JOBS",
                  "LATER_JOBS", "PULSE_JOBS", "TRACK_JOBS", "IQFIX_JOBS")     # TABLES covers ALL_, EVERY_, WHOLE_ and *_JOB_TABLES


@pytest.fixture(scope="module")
def mods():
    load_pkg()
    return {r.module: importlib.import_module("prgs-sdr-kspecanal_amd." + r.module) for r in COMPANIONS}


def test_the_registry_names_every_companion_and_the_refusals_differ():
    assert [r.so for r in COMPANIONS] == [name for name, _ in PRODUCTS[2:]] and set(SURFACE) <= set(BY_MODULE)
    assert [(r.src_dir, r.api, r.header) for r in COMPANIONS] == [row[:3] for _, row in PRODUCTS[2:]]
    assert len({r.refusal for r in COMPANIONS}) == len({r.prefix for r in COMPANIONS}) == len(COMPANIONS) == 11
    for m, (file_name, prefix, _, _) in SURFACE.items():
        assert (BY_MODULE[m].so, BY_MODULE[m].prefix) == (file_name, prefix), m


def _last_errors(mods):
    return {r.module: getattr(mods[r.module].lib(), r.prefix + "last_error")().decode() for r in COMPANIONS}


def test_every_library_keeps_its_own_thread_local_error_string(mods):
    for r in COMPANIONS:
        h = C.c_void_p(1)
        assert r.refuse(mods[r.module].lib(), C.byref(h)) != 0 and h.value is None, r.module
        assert _last_errors(mods)[r.module] == r.refusal, r.module
    # all have failed by now, each after its predecessors: none has overwritten another's text
    assert _last_errors(mods) == {r.module: r.refusal for r in COMPANIONS}
    seen = {}
    t = threading.Thread(target=lambda: seen.update(_last_errors(mods)))
    t.start()
    t.join()
    assert seen == {r.module: "" for r in COMPANIONS}, seen
    assert _last_errors(mods) == {r.module: r.refusal for r in COMPANIONS}
    # check() raises the library's own text
    for r in COMPANIONS:
        with pytest.raises(mods[r.module].KsaError, match=re.escape(r.refusal)):
            mods[r.module].check(r.refuse(mods[r.module].lib(), C.byref(C.c_void_p())))


def _header_names(r):
    return set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % r.prefix, open(os.path.join(ROOT, "include", r.header)).read()))


def test_nothing_of_the_shared_header_is_exported(mods):
    for r in COMPANIONS:
        defined = exported(r)
        leaked = [(t, name) for t, name in defined if t in "TWVBD"
                  and any(w in name for w in ("fail", "g_err", "DeviceGuard", "check_taps", "ceil_div", "check_iq_format",
                                              "check_u8_scaling", "check_device"))]
        assert not leaked, (r.so, leaked)
        own = {name for t, name in defined if t == "T" and name.startswith(r.prefix)}
        assert own == _header_names(r) == set(mods[r.module].SIGNATURES), r.so
        if r.module in SURFACE:
            assert own == set(SURFACE[r.module][3]), r.so


def test_no_library_exports_and_no_binding_holds_a_name_of_another(mods):
    lib = importlib.import_module("prgs-sdr-kspecanal_amd._lib")
    for r in COMPANIONS:
        others = tuple(p for p in PREFIXES if p != r.prefix)
        assert "ksa_" in others and len(others) == 11
        assert not [name for t, name in exported(r) if t == "T" and name.startswith(others)], r.so
        assert all(n.startswith(r.prefix) for n in mods[r.module].SIGNATURES), r.module
        assert not [n for n in lib.SIGNATURES if n.startswith(r.prefix)], r.module
    assert all(n.startswith("ksa_") for n in lib.SIGNATURES)


def test_the_build_table_is_one_and_every_product_depends_on_what_it_includes(mods):
    build = importlib.import_module("prgs-sdr-kspecanal_amd.build")
    real = os.path.realpath
    assert list(build.PRODUCTS.items()) == PRODUCTS
    assert list(build.JOBS) == [os.path.join(build.HERE, name) for name, _ in PRODUCTS] and len(build.JOBS) == 13
    assert build.HERE == PKG_DIR and (build.OUT, build.OUT_EXP) == tuple(build.JOBS)[:2]
    for name, (subdir, hip, header, extra) in PRODUCTS:
        src, flags, deps = build.JOBS[os.path.join(build.HERE, name)]
        assert (src, flags) == (os.path.join(build.HERE, subdir, hip), extra), name
        assert deps() == build._sources(name) and real(os.path.join(ROOT, "include", header)) in {real(f) for f in deps()}, name
    for r in COMPANIONS:
        deps = {real(f) for f in build.JOBS[os.path.join(build.HERE, r.so)][2]()}
        assert {real(f) for f in SHARED} <= deps, r.so
        assert {real(os.path.join(PKG_DIR, r.src_dir, f)) for f in (r.api, r.kernels)} <= deps, r.so
        assert real(os.path.join(ROOT, "include", r.header)) in deps, r.so
        assert build.is_stale(os.path.join(build.HERE, r.so)) in (False, True)
        assert build.is_stale(os.path.join(build.HERE, "no_such_" + r.so)), r.so
    for out in (build.OUT, build.OUT_EXP):
        deps = {real(f) for f in build.JOBS[out][2]()}
        assert not deps & {real(f) for f in SHARED}, out
        assert not [f for f in deps if "csrc_" in f], out
    assert build.sources() == build.JOBS[build.OUT][2]()
    # the tables, lists and twins that one table replaced are named nowhere
    gone = re.compile(r"\b\w*(%s)\b" % "|".join(DELETED_TABLES))
    assert not _files_with(gone) and not gone.search(open(os.path.join(ROOT, "__graft_entry__.py")).read())
    assert not [n for n in vars(build) if n != "PRODUCTS" and n != "JOBS" and ("PRODUCTS" in n or "JOBS" in n or "TABLES" in n)]


def test_the_shared_pieces_are_included_not_copied():
    for r in COMPANIONS:
        assert sorted(os.listdir(os.path.join(PKG_DIR, r.src_dir))) == [r.api, r.kernels], r.src_dir
        api, kernels = (open(os.path.join(PKG_DIR, r.src_dir, f)).read() for f in (r.api, r.kernels))
        for text in (api, kernels):
            assert "struct DeviceGuard" not in text and "thread_local" not in text and "getenv" not in text, r.src_dir
            assert "unpack_s16(" not in text and "unpack_u8(" not in text, r.src_dir
        assert '#include "../csrc_shared/ksa_host.hpp"' in api, r.api
        assert ('#include "../csrc_shared/ksa_iq.hpp"' in kernels) == r.raw_iq, r.kernels
        assert ("static_assert(%sFMT_C64 == ksa::iq::FMT_C64" % r.prefix.upper() in api) == r.raw_iq, r.api


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
    assert _files_with(r"SAMPLE_DTYPES = ") == ["_companion.py"] and _files_with(r"(?m)^FORMATS = ") == ["_companion.py"]
    assert _files_with(r"unknown fmt \[") == ["_companion.py"] and _files_with(r"process wants \[2n\]") == ["_companion.py"]
    assert _files_with(r"c_void_p\(\)\n.*_create\(") == ["engine.py"]           # the create tail: Companion._create alone
    for text in ("unknown sample format %d", "u8_scale %g must be", "u8_offset %g must be", "device %d must be >= 0"):
        assert [f for f in _files_with(re.escape(text)) if not f.startswith("csrc/")] == ["csrc_shared/ksa_host.hpp"], text


def test_the_binding_surface_is_what_it_was(mods):
    companion = importlib.import_module("prgs-sdr-kspecanal_amd._companion")
    engine = importlib.import_module("prgs-sdr-kspecanal_amd.engine")
    lib = importlib.import_module("prgs-sdr-kspecanal_amd._lib")
    for r in COMPANIONS:
        X = mods[r.module]
        if r.module in SURFACE:
            assert (r.so, r.prefix, X.ABI_VERSION, X.SIGNATURES) == SURFACE[r.module], r.module
        assert X.ABI_VERSION == 1 and X.LIB_PATH == os.path.join(PKG_DIR, r.so), r.module
        assert callable(X.load) and callable(X.lib) and callable(X.check), r.module
        assert issubclass(X.KsaError, RuntimeError) and X.KsaError is load_pkg().KsaError and X.KsaError is lib.KsaError, r.module
        assert X.lib() is X.lib() and getattr(X.lib(), r.prefix + "abi_version")() == X.ABI_VERSION, r.module
        missing = os.path.join(PKG_DIR, "no_such_" + r.so)
        with pytest.raises(X.KsaError) as e:
            X.load(missing)
        assert str(e.value) == ("%s is missing at %s -- build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950); "
                                "there is no CPU fallback" % (r.so, missing)), r.module
        cls = getattr(X, r.cls)
        assert issubclass(cls, companion.Companion) and isinstance(X._bind, companion.Binding) and cls._binding is X._bind, r.module
        assert getattr(load_pkg(), r.cls) is cls and r.cls in load_pkg().__all__, r.module
        assert X.DevArray is engine.DevArray, r.module
    for m in ("corr", "pulse", "iqfix"):
        assert mods[m].FORMATS is companion.FORMATS and mods[m].SAMPLE_DTYPES is companion.SAMPLE_DTYPES, m
    v = engine.DevArray(4096, (2, 3), None, "<i8").__cuda_array_interface__
    assert (v["typestr"], v["shape"], v["data"]) == ("<i8", (2, 3), (4096, False))
    assert engine.DevArray(4096, (5,), None).__cuda_array_interface__["typestr"] == "<f4"
