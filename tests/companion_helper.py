"""The registry of the companion libraries and the generic half of their header test -- TEST INFRASTRUCTURE beside
test_companion_host.py and the test_*_host.py of each library.  The next companion library is one more record here."""
import collections
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

PKG_DIR = os.path.join(ROOT, "prgs-sdr-kspecanal_amd")
SHARED = [os.path.join(PKG_DIR, "csrc_shared", f) for f in ("ksa_host.hpp", "ksa_iq.hpp")]

# module: of the package; so: beside it; prefix: of every exported symbol; header: under include/; src_dir with its api and
# kernels files; cls: the wrapper class; raw_iq: the kernels unpack raw IQ samples (csrc_shared/ksa_iq.hpp);
# refuse(lib, byref(handle)): a k??_create that is refused before any device is touched, with `refusal`, the whole text of it
Companion = collections.namedtuple("Companion", "module so prefix header src_dir api kernels cls raw_iq refuse refusal")

_TAPS = np.ones(16, dtype=np.float32)            # alive as long as the module: the refused creates get its address
_P = _TAPS.ctypes.data_as(C.c_void_p)


def _record(module, prefix, cls, raw_iq, refuse, refusal):
    return Companion(module, "libksa_%s.so" % module, prefix, "ksa_%s.h" % module, "csrc_" + module, prefix + "api.hip",
                     prefix + "kernels.hpp", cls, raw_iq, refuse, refusal)


COMPANIONS = [
    _record("density", "ksd_", "SpectrumDensity", False,
            lambda lib, h: lib.ksd_create(0, 1024, 0, 256, -140.0, 0.0, h), "width 0 must be >= 1"),
    _record("mask", "ksm_", "SpectrumMask", False,
            lambda lib, h: lib.ksm_create(0, 1024, None, None, 0, 16, h), "min_bins 0 must be >= 1"),
    _record("ddc", "kdc_", "DownConverter", True,
            lambda lib, h: lib.kdc_create(0, 0, 0.0, 1.0, 0, 8, _P, 0, 64, h), "decim 0 outside 1..1024"),
    _record("detect", "kse_", "SignalDetector", False,
            lambda lib, h: lib.kse_create(0, 1024, 0, 2, 10.0, 0, 1, 0, 16, h), "train 0 outside 1..1024"),
    _record("demod", "kdm_", "Demodulator", False,
            lambda lib, h: lib.kdm_create(0, 7, 4, 8, _P, 0, 1.0, 64, h), "unknown mode 7"),
    _record("chan", "kch_", "Channelizer", True,
            lambda lib, h: lib.kch_create(0, 0, 0.0, 1.0, 3, 1, 8, _P, 64, h), "nchan 3 must be a power of two, 2..1024"),
    _record("resamp", "krs_", "Resampler", False,
            lambda lib, h: lib.krs_create(0, 0, 4, 6, 4, _P, 0, 1.0, 64, h), "L / M = 4 / 6 is not reduced, use 2 / 3"),
    _record("corr", "kcr_", "Correlator", True,
            lambda lib, h: lib.kcr_create(0, 0, 127.5, 127.5, 8, 9, _P, 0.5, 0.0, 4, 16, 64, h), "Q 9 outside 1..8"),
    _record("pulse", "kpl_", "PulseDetector", True,
            lambda lib, h: lib.kpl_create(0, 0, 127.5, 127.5, 4097, 0.5, 0.25, 1, 16, 64, h), "W 4097 outside 1..4096"),
    _record("track", "ktr_", "EmissionTracker", False,
            lambda lib, h: lib.ktr_create(0, 0, 4096, 1, 2, 1, 1, 16, h), "nbins 0 outside 1..16777216"),
    _record("iqfix", "kqf_", "IqCorrector", True,
            lambda lib, h: lib.kqf_create(0, 0, 127.5, 127.5, 0, h), "max_in 0 outside 1..268435455"),
]
BY_MODULE = {r.module: r for r in COMPANIONS}
PREFIXES = ("ksa_",) + tuple(r.prefix for r in COMPANIONS)


def exported(record):
    """[(type letter, name)] of the dynamic symbols the library defines, demangled."""
    nm = subprocess.run(["nm", "-D", "--defined-only", "-C", os.path.join(PKG_DIR, record.so)], capture_output=True, text=True)
    assert nm.returncode == 0, nm.stderr
    fields = [ln.split(None, 2) for ln in nm.stdout.splitlines()]
    return [(f[1], f[2]) for f in fields if len(f) == 3]


def check_header_exports_binding(record, module, tmp_path, extra_c="", macros=()):
    """What every library's header test checks alike: the header compiles as pedantic C99 with every k??_ name it holds taken
    as a function, with extra_c (struct sizes, offsets, the handle type) and with every expression of macros; those names are
    the library's exported functions of its prefix and the binding's SIGNATURES; no function of another library's prefix or of
    libksa's is exported; the header's ABI version is the binding's.  Returns (the header's text, the names)."""
    text = open(os.path.join(ROOT, "include", record.header)).read()
    names = sorted(set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % record.prefix, text)))
    stem = "use_" + record.prefix.rstrip("_")
    src = tmp_path / (stem + ".c")
    src.write_text('#include "%s"\n#include <stddef.h>\n' % record.header
                   + 'typedef void (*fn_t)(void);\nstatic const fn_t table[] = {' + ", ".join("(fn_t)%s" % n for n in names) + '};\n'
                   + extra_c
                   + 'int %s(void) { return (int)sizeof(table) + %s; }\n' % (stem, " + ".join(("%sABI_VERSION" % record.prefix.upper(),) + tuple(macros))))
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / (stem + ".o"))], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    symbols = [name for t, name in exported(record) if t == "T"]
    own = {s for s in symbols if s.startswith(record.prefix)}
    assert own == set(names), own ^ set(names)
    assert set(module.SIGNATURES) == set(names), set(module.SIGNATURES) ^ set(names)
    others = tuple(p for p in PREFIXES if p != record.prefix)
    assert not [s for s in symbols if s.startswith(others)], "the companion library must not shadow the others"
    assert int(re.search(r"#define %sABI_VERSION (\d+)" % record.prefix.upper(), text).group(1)) == module.ABI_VERSION
    return text, names
