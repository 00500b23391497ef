#!/usr/bin/env python3
"""Spectrum-stage timing of one shape (complex64 input): bench_one.py N nonOverlap window fullSize frames [fold]
fold: AVG (default) | MAX | MIN | PSD -- the engine's cumu_mode (tools/psd_sweep.py alternates AVG and PSD through run())."""
import importlib, os, sys, json
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ksa_oracle as orc
ksa = importlib.import_module("prgs-sdr-kspecanal_amd")


def run(n, q, win, full, frames, fold="AVG", launches=5):
    """Mean spectrum-stage time (ksa_prof_read) of `launches` curscan_dev calls in dB units: (ms, windows per frame, VGPRs)."""
    distinct = min(frames, max(1, (64 << 20) // (full * 8)))
    host = orc.synth_iq(full * distinct, 1 + n).astype(np.complex64)
    tile = torch.view_as_real(torch.from_numpy(host)).reshape(distinct, full, 2).cuda()
    iq = tile.repeat((frames + distinct - 1) // distinct, 1, 1)[:frames].contiguous()
    # (xres = N: any fftSize, 2^a*3^b*5^c included, has a valid waterfall width; curscan_dev writes no waterfall)
    eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window=win, xres=n, max_frames=frames, cumu_mode=fold,
                             stream=torch.cuda.current_stream().cuda_stream)
    out = torch.empty((frames, n), dtype=torch.float32, device="cuda")
    for _ in range(2): eng.curscan_dev(iq, ksa.FMT_C64, frames, out, out_mode=ksa.OUT_DB)
    torch.cuda.synchronize(); eng.prof_enable(True)
    for _ in range(launches): eng.curscan_dev(iq, ksa.FMT_C64, frames, out, out_mode=ksa.OUT_DB)
    ms, k = eng.prof_read()
    res = (ms / k, eng.num_windows, eng.kernel_info()["vgprs"])
    eng.close()
    return res


if __name__ == "__main__":
    n, q, win, full, frames = int(sys.argv[1]), float(sys.argv[2]), sys.argv[3], int(sys.argv[4]), int(sys.argv[5])
    fold = sys.argv[6].upper() if len(sys.argv) > 6 else "AVG"
    ms, nwin, vgprs = run(n, q, win, full, frames, fold)
    tag = os.environ.get("KSA_VARIANT", "main") + ("" if fold == "AVG" else " " + fold)
    print("%s N=%d q=%s: %.3f ms  %.2f MFFT/s  vgpr %d" % (tag, n, q, ms, frames * nwin / ms / 1e3, vgprs))
