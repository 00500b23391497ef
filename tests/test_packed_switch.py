"""The A/B switch of the packed butterflies (KSA_PLAIN) exists in the experiments build only: the product library
neither reads the variable nor carries the plain instantiation of the kernels that ship packed (host test, no GPU)."""
import importlib
import os
import re

from conftest import ROOT, load_pkg

CSRC = os.path.join(ROOT, "prgs-sdr-kspecanal_amd", "csrc")


def test_the_product_library_has_no_plain_switch():
    load_pkg()
    lib_mod = importlib.import_module("prgs-sdr-kspecanal_amd._lib")
    product = open(lib_mod.LIB_PATH, "rb").read()
    exp = open(os.path.join(os.path.dirname(lib_mod.LIB_PATH), "libksa_exp.so"), "rb").read()
    for needle in (b"KSA_PLAIN", b"spectrum_plain_kernel"):
        assert needle not in product, "libksa.so holds %r" % needle
        assert needle in exp, "libksa_exp.so lacks %r: the switch is gone from the experiments build as well" % needle


def test_the_switch_is_read_through_exp_env_and_compiled_under_ksa_experiments():
    api = open(os.path.join(CSRC, "ksa_api.hip")).read()
    assert 'exp_env("KSA_PLAIN")' in api and 'getenv("KSA_PLAIN")' not in api
    for src in (api, open(os.path.join(CSRC, "ksa_kernels.hpp")).read()):
        for m in re.finditer(r"spectrum_plain_kernel", src):
            head = src[:m.start()]
            assert head.rfind("#ifdef KSA_EXPERIMENTS") > head.rfind("#endif"), "spectrum_plain_kernel outside #ifdef KSA_EXPERIMENTS"
