"""Build libksa.so (HIP kernels + C ABI) for gfx950 with hipcc.  In-tree, no JIT cache:
the .so sits next to this file so that it travels to the GPU box with the repo snapshot.
Beside it libksa_exp.so, the same sources with -DKSA_EXPERIMENTS: the only build that reads the KSA_* environment
switches (tests/test_gpu_tickets.py runs both unit orders of the spectrum kernel through it); the package never loads it.
And libksa_density.so, libksa_mask.so and libksa_ddc.so, the companion libraries of include/ksa_density.h, include/ksa_mask.h
and include/ksa_ddc.h, each from its own sources under csrc_density/, csrc_mask/ and csrc_ddc/.
And libksa_detect.so, the CFAR signal detector of include/ksa_detect.h, from csrc_detect/.
And libksa_demod.so, the AM / FM / PM demodulator of include/ksa_demod.h, from csrc_demod/.
And libksa_chan.so, the polyphase channelizer of include/ksa_chan.h, from csrc_chan/."""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "ksa_api.hip")
OUT = os.path.join(HERE, "libksa.so")
OUT_EXP = os.path.join(HERE, "libksa_exp.so")
SRC_DENSITY = os.path.join(HERE, "csrc_density", "ksd_api.hip")
OUT_DENSITY = os.path.join(HERE, "libksa_density.so")
SRC_MASK = os.path.join(HERE, "csrc_mask", "ksm_api.hip")
OUT_MASK = os.path.join(HERE, "libksa_mask.so")
SRC_DDC = os.path.join(HERE, "csrc_ddc", "kdc_api.hip")
OUT_DDC = os.path.join(HERE, "libksa_ddc.so")
SRC_DETECT = os.path.join(HERE, "csrc_detect", "kse_api.hip")
OUT_DETECT = os.path.join(HERE, "libksa_detect.so")
SRC_DEMOD = os.path.join(HERE, "csrc_demod", "kdm_api.hip")
OUT_DEMOD = os.path.join(HERE, "libksa_demod.so")
SRC_CHAN = os.path.join(HERE, "csrc_chan", "kch_api.hip")
OUT_CHAN = os.path.join(HERE, "libksa_chan.so")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-Wno-unused-value",
         "-shared", "-fPIC"]


def _tree(subdir, header):
    d = os.path.join(HERE, subdir)
    return [os.path.join(d, f) for f in sorted(os.listdir(d))] + [os.path.join(HERE, "..", "include", header)]


def sources():
    return _tree("csrc", "ksa.h")


def density_sources():
    return _tree("csrc_density", "ksa_density.h")


def mask_sources():
    return _tree("csrc_mask", "ksa_mask.h")


def ddc_sources():
    return _tree("csrc_ddc", "ksa_ddc.h")


def detect_sources():
    return _tree("csrc_detect", "ksa_detect.h")


def demod_sources():
    return _tree("csrc_demod", "ksa_demod.h")


def chan_sources():
    return _tree("csrc_chan", "ksa_chan.h")


# product -> (the .hip that is compiled, extra flags, every file the product depends on)
JOBS = {
    OUT: (SRC, [], sources),
    OUT_EXP: (SRC, ["-DKSA_EXPERIMENTS"], sources),
    OUT_DENSITY: (SRC_DENSITY, [], density_sources),
    OUT_MASK: (SRC_MASK, [], mask_sources),
    OUT_DDC: (SRC_DDC, [], ddc_sources),
    OUT_DETECT: (SRC_DETECT, [], detect_sources),
    OUT_DEMOD: (SRC_DEMOD, [], demod_sources),
    OUT_CHAN: (SRC_CHAN, [], chan_sources),
}


def is_stale(out=OUT):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(s) > t for s in JOBS[out][2]())


def build(force=False, verbose=False):
    """Compile what is missing or older than its sources (the eight libraries side by side).  Returns the product's path."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    jobs = []
    for out, (src, extra, _) in JOBS.items():
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
