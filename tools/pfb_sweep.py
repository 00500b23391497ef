#!/usr/bin/env python3
"""Polyphase front end (pfb_taps) against the transform stage alone: pfb_sweep.py [repeats] [main|ring|chunk] >> profiles/pfb_sweep.txt

One process, one GPU.  Frames advance by N samples over one stream held in device memory (the critically sampled PFB).  Per case
the PFB engine and an AVG engine of the same build with ONE window per frame (full_size = N, non_overlap = 1, rectangular
window: the transform stage alone, on the kernels the fold hands its frames to) alternate `repeats` times; a run is the time of
`LAUNCHES` curscan_dev calls between two events on the engine's stream, in dB units.  Medians, min and max are printed.

  main   N = 4096 and 64, P = 4 and 8, complex64 and uint8: PFB against AVG.
  ring   (a) the ring kernel against the generic kernel at stride N, for the cases above and for P = 16 and the int8 / int16
         formats.  Needs an experiments build (tools/variants.sh; run through tools/with_lib.sh): only such a build reads
         KSA_PFB_NO_RING, which this mode sets and clears between runs.  A (format, P) pair that the library never hands to the
         ring kernel ((P - 1) * bytes per sample < 12) runs the generic kernel on both sides and reads 1.00.
  chunk  (b) the PFB cases alone, labelled with the library in use: run once per build of -DKSA_PFB_CHUNK_BYTES=16 / 64 / 256 MiB.
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
STREAM_BYTES = 256 << 20          # complex64 stream per case: the folded frames of one call fill one 256 MiB chunk
CASES = [(n, p, fmt) for n in (4096, 64) for p in (4, 8) for fmt in ("c64", "u8")]
RING_EXTRA = [(4096, 16, "c64"), (4096, 16, "u8"), (4096, 4, "s16"), (4096, 8, "s16"), (4096, 8, "s8"), (64, 16, "c64"), (64, 16, "u8")]
FMT = {"c64": ksa.FMT_C64, "u8": ksa.FMT_U8, "s8": ksa.FMT_S8, "s16": ksa.FMT_S16}


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
    def __init__(self, n, p, fmt):
        self.n, self.p, self.fmt = n, p, fmt
        self.frames = STREAM_BYTES // (8 * n)
        self.code = FMT[fmt]
        self.iq = _stream((self.frames + p) * n, fmt, 1 + n + p)
        self.out = torch.empty((self.frames, n), dtype=torch.float32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        self.pfb = ksa.SpectrumEngine(n, pfb_taps=p, window="hamming", xres=min(n, 512), max_frames=self.frames, stream=stream)
        self.avg = ksa.SpectrumEngine(n, full_size=n, non_overlap=1.0, window="ones", cumu_mode="AVG", xres=min(n, 512),
                                      max_frames=self.frames, stream=stream)
        for eng in (self.pfb, self.avg):
            self.run(eng)

    def run(self, eng):
        """M spectra per second over LAUNCHES calls."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(LAUNCHES):
            eng.curscan_dev(self.iq, self.code, self.frames, self.out, out_mode=ksa.OUT_DB, frame_stride=self.n)
        b.record()
        torch.cuda.synchronize()
        return self.frames * LAUNCHES / a.elapsed_time(b) / 1e3

    def close(self):
        self.pfb.close()
        self.avg.close()


def _row(label, v):
    return "  %-34s %9.2f %9.2f %9.2f" % (label, min(v), statistics.median(v), max(v))


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    mode = sys.argv[2] if len(sys.argv) > 2 else "main"
    lib = os.environ.get("KSA_VARIANT", "main")
    if mode == "main":
        print("# pfb_taps against the AVG fold with one window per frame (the transform stage alone), frames at stride N, dB output,")
        print("# one MI355X, library %s; the two engines alternate %d times, %d launches per run.  M spectra / s." % (lib, repeats, LAUNCHES))
        print("# %-34s %9s %9s %9s | %s" % ("case", "min", "median", "max", "PFB / AVG (medians)"))
    elif mode == "ring":
        print("# (a) ring kernel against generic kernel at stride N (KSA_PFB_NO_RING on an experiments build), library %s," % lib)
        print("# alternating %d times.  M spectra / s.  Kept: the ring median beats the generic median by more than both spreads." % repeats)
        print("# %-34s %9s %9s %9s | %s" % ("case", "min", "median", "max", "ring / generic (medians), verdict"))
    else:
        print("# (b) library %s: PFB cases alone, %d runs.  M spectra / s." % (lib, repeats))
    for n, p, fmt in CASES + (RING_EXTRA if mode == "ring" else []):
        c = Case(n, p, fmt)
        name = "N=%d P=%d %s %d frames" % (n, p, fmt, c.frames)
        if mode == "main":
            r = {"PFB": [], "AVG": []}
            for _ in range(repeats):
                for k, eng in (("PFB", c.pfb), ("AVG", c.avg)):
                    r[k].append(c.run(eng))
            print(_row(name + " AVG", r["AVG"]) + " |")
            print(_row(name + " PFB", r["PFB"]) + " | %.3f" % (statistics.median(r["PFB"]) / statistics.median(r["AVG"])))
        elif mode == "ring":
            r = {"ring": [], "generic": []}
            for _ in range(repeats):
                for k in ("ring", "generic"):
                    if k == "generic":
                        os.environ["KSA_PFB_NO_RING"] = "1"
                    else:
                        os.environ.pop("KSA_PFB_NO_RING", None)
                    r[k].append(c.run(c.pfb))
            os.environ.pop("KSA_PFB_NO_RING", None)
            mr, mg = statistics.median(r["ring"]), statistics.median(r["generic"])
            spread = (max(r["ring"]) - min(r["ring"])) + (max(r["generic"]) - min(r["generic"]))
            verdict = "ring faster" if mr - mg > spread else "generic faster" if mg - mr > spread else "within the spread"
            print(_row(name + " generic", r["generic"]) + " |")
            print(_row(name + " ring", r["ring"]) + " | %.3f %s" % (mr / mg, verdict))
        else:
            print(_row(name + " PFB " + lib, [c.run(c.pfb) for _ in range(repeats)]))
        sys.stdout.flush()
        c.close()
        del c
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
