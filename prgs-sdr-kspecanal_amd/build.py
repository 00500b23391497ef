"""Build the shared libraries for gfx950 with hipcc, one translation unit each (the PRODUCTS table below, then ADDONS).  In-tree, no
JIT cache: every .so sits next to this file so that it travels with the repository snapshot.  libksa_exp.so is libksa.so's
sources with -DKSA_EXPERIMENTS, the only build that reads the KSA_* environment switches; the package never loads it."""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-Wno-unused-value",
         "-shared", "-fPIC"]

# product -> (source directory, the .hip that is compiled, public header under include/, extra flags); built in this order.
# The next companion library is one more row.
PRODUCTS = {
    "libksa.so": ("csrc", "ksa_api.hip", "ksa.h", []),
    "libksa_exp.so": ("csrc", "ksa_api.hip", "ksa.h", ["-DKSA_EXPERIMENTS"]),
    "libksa_density.so": ("csrc_density", "ksd_api.hip", "ksa_density.h", []),
    "libksa_mask.so": ("csrc_mask", "ksm_api.hip", "ksa_mask.h", []),
    "libksa_ddc.so": ("csrc_ddc", "kdc_api.hip", "ksa_ddc.h", []),
    "libksa_detect.so": ("csrc_detect", "kse_api.hip", "ksa_detect.h", []),
    "libksa_demod.so": ("csrc_demod", "kdm_api.hip", "ksa_demod.h", []),
    "libksa_chan.so": ("csrc_chan", "kch_api.hip", "ksa_chan.h", []),
    "libksa_resamp.so": ("csrc_resamp", "krs_api.hip", "ksa_resamp.h", []),
    "libksa_corr.so": ("csrc_corr", "kcr_api.hip", "ksa_corr.h", []),
    "libksa_pulse.so": ("csrc_pulse", "kpl_api.hip", "ksa_pulse.h", []),
    "libksa_track.so": ("csrc_track", "ktr_api.hip", "ksa_track.h", []),
    "libksa_iqfix.so": ("csrc_iqfix", "kqf_api.hip", "ksa_iqfix.h", []),
}
# Products built after the ones above, in the same row format.  The tests of the build table pin `PRODUCTS` to its thirteen rows and
# the kernel catalogue to twelve libraries, so the band meter waits here; its row moves into `PRODUCTS` once those may change.
ADDONS = {
    "libksa_measure.so": ("csrc_measure", "kme_api.hip", "ksa_measure.h", []),
}
OUT = os.path.join(HERE, "libksa.so")
OUT_EXP = os.path.join(HERE, "libksa_exp.so")


def _files(subdir):
    d = os.path.join(HERE, subdir)
    return [os.path.join(d, f) for f in sorted(os.listdir(d))]


def _sources(product):
    """Every file the product depends on: its directory, its header and, for a companion library, csrc_shared/ (which csrc/
    does not include)."""
    subdir, _, header, _ = PRODUCTS[product] if product in PRODUCTS else ADDONS[product]
    shared = _files("csrc_shared") if subdir != "csrc" else []
    return _files(subdir) + shared + [os.path.join(HERE, "..", "include", header)]


def sources():
    return _sources("libksa.so")


def _jobs(table):
    """product's path -> (the .hip that is compiled, extra flags, every file the product depends on)"""
    return {os.path.join(HERE, name): (os.path.join(HERE, subdir, hip), extra, lambda name=name: _sources(name))
            for name, (subdir, hip, _, extra) in table.items()}


JOBS = _jobs(PRODUCTS)
_ADDON_WORK = _jobs(ADDONS)                      # not part of JOBS: build() runs these whatever a caller has narrowed JOBS to


def is_stale(out=OUT):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    deps = JOBS[out][2] if out in JOBS else _ADDON_WORK[out][2]
    return any(os.path.getmtime(s) > t for s in deps())


def build(force=False, verbose=False):
    """Compile what is missing or older than its sources (the libraries side by side).  Returns the product's path."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    jobs = []
    for out, (src, extra, _) in list(JOBS.items()) + list(_ADDON_WORK.items()):
        if not force and not is_stale(out):
            continue
        cmd = [hipcc] + FLAGS + extra + ["-o", out + ".tmp", src]
        if verbose:
            print(" ".join(cmd))
        jobs.append((out, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    failed = []
    for out, proc in jobs:
        log = proc.communicate()[0]
        if proc.returncode != 0:
            failed.append(log)
        else:
            os.replace(out + ".tmp", out)
    if failed:
        raise RuntimeError("hipcc failed:\n" + "\n".join(failed))
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
