#!/usr/bin/env python3
"""Integrating polyphase spectrometer (pfb_taps + pfb_spectra) against what the polyphase front end alone offers for the same
spectra: pfbpsd_sweep.py [repeats] [main|ring] >> profiles/pfbpsd_sweep.txt

One process, one GPU, one sample stream per shape in device memory.  The KSA_CUMU_PFB_PSD engine reads `blocks` blocks of
(P+K-1)*N samples at stride K*N and writes one integrated spectrum per block; the KSA_CUMU_PFB engine reads the same stream at
stride N and writes the blocks*K spectra a caller would then have to square and sum.  Both in dB units, the spectrum stage timed
by the profiling entry points (fold + transform of every chunk), `LAUNCHES` calls per run; the engines alternate `repeats` times.
Reported: ns per polyphase spectrum (a sub-frame), min / median / max.

  main   the shapes of DESIGN 4.10.  Bar: the integrating engine's median is not above the front end's median plus the front
         end's own max - min.
  ring   the block ring kernel against the block generic kernel per (format, P).  Needs an experiments build (tools/variants.sh;
         run through tools/with_lib.sh): only such a build reads KSA_PFB_NO_RING, which this mode sets and clears between runs.
"""
import importlib
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ksa_oracle as orc  # noqa: E402

ksa = importlib.import_module("prgs-sdr-kspecanal_amd")

LAUNCHES = 3
FMT = {"c64": ksa.FMT_C64, "u8": ksa.FMT_U8, "s8": ksa.FMT_S8, "s16": ksa.FMT_S16}
# (N, P, K, format, blocks): blocks*K folded sub-frames fill at most one 256 MiB chunk on either engine
SHAPES = [(4096, 4, 16, "c64", 512), (4096, 4, 16, "s16", 512), (1024, 8, 64, "c64", 512), (65536, 4, 8, "c64", 64),
          (2400, 4, 16, "c64", 512)]
RING_EXTRA = [(4096, 8, 16, "u8", 512), (4096, 8, 16, "s8", 512), (4096, 8, 16, "s16", 512), (4096, 16, 16, "c64", 512),
              (4096, 16, 16, "u8", 512), (4096, 16, 16, "s8", 512), (4096, 16, 16, "s16", 512), (4096, 4, 16, "u8", 512),
              (4096, 4, 16, "s8", 512), (64, 4, 16, "c64", 32768), (64, 4, 16, "u8", 32768), (64, 4, 16, "s8", 32768),
              (64, 8, 64, "u8", 8192), (64, 16, 16, "c64", 32768), (4096, 4, 2, "u8", 4096), (4096, 4, 1, "u8", 8192)]


def _stream(samples, fmt, seed):
    """`samples` IQ samples on the device: one 2^20-sample draw of the oracle's generator, repeated."""
    base = (orc.synth_iq(1 << 20, seed) * 0.7).astype(np.complex64)
    if fmt != "c64":
        if fmt == "u8":
            q = orc.quantize_u8(base)
        else:
            bits, dtype = (7, np.int8) if fmt == "s8" else (15, np.int16)
            q = np.clip(np.round(base.view(np.float32).astype(np.float64) * (1 << bits)), -(1 << bits), (1 << bits) - 1).astype(dtype)
        t = torch.from_numpy(q).cuda()
        return t.repeat(-(-2 * samples // t.numel()))[:2 * samples].contiguous()
    t = torch.view_as_real(torch.from_numpy(base)).cuda()
    return t.repeat(-(-samples // t.shape[0]), 1)[:samples].contiguous()


class Case:
    def __init__(self, n, p, k, fmt, blocks, front_end=True):
        self.n, self.p, self.k, self.blocks, self.code = n, p, k, blocks, FMT[fmt]
        self.iq = _stream((blocks * k + p) * n, fmt, 1 + n + p)
        stream = torch.cuda.current_stream().cuda_stream
        xres = n if n & (n - 1) else min(n, 512)
        self.six = ksa.SpectrumEngine(n, pfb_taps=p, pfb_spectra=k, window="hamming", xres=xres, max_frames=blocks, stream=stream)
        self.out6 = torch.empty((blocks, n), dtype=torch.float32, device="cuda")
        self.five = self.out5 = None
        if front_end:
            self.five = ksa.SpectrumEngine(n, pfb_taps=p, window="hamming", xres=xres, max_frames=blocks * k, stream=stream)
            self.out5 = torch.empty((blocks * k, n), dtype=torch.float32, device="cuda")
        for eng in (self.six, self.five):
            if eng is not None:
                self.run(eng)

    def run(self, eng):
        """ns per polyphase spectrum: the profiled spectrum stages of LAUNCHES calls."""
        eng.prof_enable(True)       # (clears the events of the run before)
        for _ in range(LAUNCHES):
            if eng is self.six:
                eng.curscan_dev(self.iq, self.code, self.blocks, self.out6, out_mode=ksa.OUT_DB, frame_stride=self.k * self.n)
            else:
                eng.curscan_dev(self.iq, self.code, self.blocks * self.k, self.out5, out_mode=ksa.OUT_DB, frame_stride=self.n)
        ms, _ = eng.prof_read()
        return ms * 1e6 / (LAUNCHES * self.blocks * self.k)

    def close(self):
        self.six.close()
        if self.five is not None:
            self.five.close()


def _row(label, v, tail=""):
    return "  %-44s %9.3f %9.3f %9.3f | %s" % (label, min(v), statistics.median(v), max(v), tail)


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    mode = sys.argv[2] if len(sys.argv) > 2 else "main"
    lib = os.environ.get("KSA_VARIANT", "main")
    if mode == "main":
        print("# pfb_spectra (KSA_CUMU_PFB_PSD, one row per block) against pfb_taps alone at stride N (KSA_CUMU_PFB, one row per spectrum),")
        print("# the same stream, dB output, one MI355X, library %s; the engines alternate %d times, %d launches per run." % (lib, repeats, LAUNCHES))
        print("# ns per polyphase spectrum.  Bar: median(PFB_PSD) <= median(PFB) + (max - min)(PFB).")
        print("# %-44s %9s %9s %9s | %s" % ("shape", "min", "median", "max", "PFB_PSD / PFB (medians), verdict"))
    else:
        print("# block ring kernel against block generic kernel (KSA_PFB_NO_RING on an experiments build), library %s," % lib)
        print("# alternating %d times, %d launches per run.  ns per polyphase spectrum, fold + transform." % (repeats, LAUNCHES))
        print("# %-44s %9s %9s %9s | %s" % ("shape", "min", "median", "max", "generic / ring (medians), verdict"))
    for n, p, k, fmt, blocks in SHAPES + (RING_EXTRA if mode == "ring" else []):
        c = Case(n, p, k, fmt, blocks, front_end=mode == "main")
        name = "N=%d P=%d K=%d %s %d blocks" % (n, p, k, fmt, blocks)
        if mode == "main":
            r = {"PFB_PSD": [], "PFB": []}
            for _ in range(repeats):
                for key, eng in (("PFB_PSD", c.six), ("PFB", c.five)):
                    r[key].append(c.run(eng))
            m6, m5 = statistics.median(r["PFB_PSD"]), statistics.median(r["PFB"])
            spread = max(r["PFB"]) - min(r["PFB"])
            print(_row(name + " PFB", r["PFB"], "(spread %.3f)" % spread))
            print(_row(name + " PFB_PSD", r["PFB_PSD"], "%.3f %s" % (m6 / m5, "ok" if m6 <= m5 + spread else "SLOWER than PFB + its spread")))
        else:
            r = {"ring": [], "generic": []}
            for _ in range(repeats):
                for key in ("ring", "generic"):
                    if key == "generic":
                        os.environ["KSA_PFB_NO_RING"] = "1"
                    else:
                        os.environ.pop("KSA_PFB_NO_RING", None)
                    r[key].append(c.run(c.six))
            os.environ.pop("KSA_PFB_NO_RING", None)
            mr, mg = statistics.median(r["ring"]), statistics.median(r["generic"])
            spread = (max(r["ring"]) - min(r["ring"])) + (max(r["generic"]) - min(r["generic"]))
            verdict = "ring faster" if mg - mr > spread else "generic faster" if mr - mg > spread else "within the spread"
            print(_row(name + " generic", r["generic"]))
            print(_row(name + " ring", r["ring"], "%.3f %s" % (mg / mr, verdict)))
        sys.stdout.flush()
        c.close()
        del c
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
