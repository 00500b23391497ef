"""The kernel catalogue against what is compiled (CPU suite): the kernel names of every shipped library's gfx950 code object
must equal the names of tests/kernel_catalogue.py, in both directions and by name, so that a template instantiation added to a
dispatcher cannot ship without a record that says which reference-checked test launches it.

The names come from the built libraries: the gfx950 code object is taken out of each library's fat binary and its kernel
descriptor symbols (`<name>.kd`) are read and demangled.  Only names are read, no instruction text.  build() comes first, as for
every test that loads the package; run on its own in a tree without the libraries, the test builds the twelve in scope and
nothing else (not libksa_exp.so), so it never compiles ksa_api.hip when build() has run and once when it has not."""
import copy
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

import kernel_catalogue as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "prgs-sdr-kspecanal_amd")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def _build_module():
    spec = importlib.util.spec_from_file_location("ksa_build_for_catalogue", os.path.join(PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _llvm(tool):
    """An LLVM tool of the ROCm installation hipcc belongs to."""
    hipcc = os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc")
    rocm = os.path.dirname(os.path.dirname(hipcc))
    for d in (os.path.join(rocm, "lib", "llvm", "bin"), os.path.join(rocm, "llvm", "bin"), os.path.dirname(hipcc)):
        if os.path.exists(os.path.join(d, tool)):
            return os.path.join(d, tool)
    found = shutil.which(tool)
    assert found, "no %s beside hipcc (%s) or on PATH" % (tool, hipcc)
    return found


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, (cmd, r.stderr[-2000:])
    return r.stdout


def kernel_names(lib_path, workdir):
    """Demangled, shortened names of the kernels in the gfx950 code object of one shared library."""
    base = os.path.join(str(workdir), os.path.basename(lib_path))
    _run([_llvm("llvm-objcopy"), "--dump-section", ".hip_fatbin=%s.fatbin" % base, lib_path, base + ".copy"])
    _run([_llvm("clang-offload-bundler"), "--unbundle", "--type=o", "--input=%s.fatbin" % base, "--targets=" + TARGET,
          "--output=%s.co" % base])
    table = _run([_llvm("llvm-readelf"), "--symbols", "--wide", base + ".co"])
    mangled = sorted({m.group(1) for m in re.finditer(r"\s(\S+)\.kd\s*$", table, flags=re.M)})
    assert mangled, "no kernel descriptor in " + lib_path
    demangled = _run(["c++filt"] + mangled).split("\n")[:len(mangled)]
    return {kc.short_name(d) for d in demangled}


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    build = _build_module()
    libs = [name for name in build.PRODUCTS if name != "libksa_exp.so"]
    assert len(libs) == 12
    build.JOBS = build._jobs({name: build.PRODUCTS[name] for name in libs})      # (this module object is the test's own)
    build.build(force=False)
    work = tmp_path_factory.mktemp("code_objects")
    return {name: kernel_names(os.path.join(PKG, name), work) for name in libs}


def test_every_compiled_kernel_has_a_record_and_every_record_a_kernel(compiled):
    msgs = kc.compare(compiled, kc.by_library())
    assert not msgs, "\n".join(msgs)
    assert sum(len(v) for v in compiled.values()) == len(kc.RECORDS), "a kernel is listed twice"


def test_the_comparison_fails_by_name_when_a_record_or_a_kernel_is_missing(compiled):
    victim = next(r for r in kc.RECORDS if r["kernel"] == "ksa::ddc::tile_kernel<0, 2>")
    base = kc.compare(compiled, kc.by_library())           # (empty unless the first test fails too)
    fewer = [copy.deepcopy(r) for r in kc.RECORDS if r is not victim]
    new = [m for m in kc.compare(compiled, kc.by_library(fewer)) if m not in base]
    assert new == ["libksa_ddc.so: kernel ksa::ddc::tile_kernel<0, 2> has no catalogue entry"]
    more = kc.RECORDS + [dict(lib="libksa_mask.so", kernel="ksa::mask::check_kernel<2>", recipe=("mask", 2))]
    new = [m for m in kc.compare(compiled, kc.by_library(more)) if m not in base]
    assert new == ["libksa_mask.so: entry ksa::mask::check_kernel<2> matches nothing"]


def test_records_are_well_formed_and_name_tests_that_exist():
    seen = set()
    for r in kc.RECORDS:
        kind = kc.kind_of(r)
        assert (r["lib"], r["kernel"]) not in seen, r
        seen.add((r["lib"], r["kernel"]))
        nodes = r[kind] if kind == "covered_by" else (r[kind],) if kind == "exempt" else ()
        for node in nodes:
            path, func = node.split("::")
            text = open(os.path.join(ROOT, path)).read()
            assert re.search(r"^def %s\(" % re.escape(func), text, flags=re.M), node
            assert "pytest.mark.gpu" in text, path
        if kind == "covered_by":
            assert "<" not in r["kernel"], "a templated kernel needs a recipe: %s" % r["kernel"]
        if kind == "unreachable":
            assert "ksa_api.hip" in r[kind] and r["kernel"].startswith("ksa::spectrum_kernel<64, 0, 0, ")
    assert [r["kernel"] for r in kc.RECORDS if "exempt" in r] == ["ksa::clock_stamp_kernel"]
    assert len([r for r in kc.RECORDS if "unreachable" in r]) == 4
