"""Packed fp32 butterflies: the ping-pong 50 %-overlap kernels of N = 4096 run their butterflies as v_pk_add_f32 /
v_pk_mul_f32 / v_pk_fma_f32 on the (re, im) pair of one complex value (ksa_fft.hpp, policy Packed).  The packed forms perform the
same FMAs in the same order on the same operands as the plain ones, so the two instantiations must give the SAME BITS.

Every case runs one input through the experiments build (libksa_exp.so; only it reads environment switches) twice: as shipped
and with KSA_PLAIN=1, the plain instantiation of the same kernel.  KSA_NO_SPLIT=1 keeps whole frames as units, so that a frame of
W windows walks the two-window loop as W says (both parities, the odd tail, the first window that loads all 16 samples); one
case runs the window split as well.  Compared, as bit patterns (NaNs in equal places included): the per-frame dB rows (cur_db),
the waterfall rows (hm_rows), Cur / Max / Min / Avg and the ring.

Shapes: N = 4096 at 50 % overlap, full_size = 4096 + 2048 (W - 1) for W = 1, 2, 3, 4, 15; 5 frames; xres 512; AVG, MAX, MIN and PSD
folds; complex64, uint8, int8 and int16 input; a NaN sample, a +-inf sample, an all-zero frame, samples of about 1e-38."""
import importlib
import os

import numpy as np
import pytest

import ksa_oracle as orc

pytestmark = pytest.mark.gpu

SWITCHES = ("KSA_PLAIN", "KSA_NO_SPLIT")
N, NFRAMES, XRES = 4096, 5, 512
WINDOWS = (1, 2, 3, 4, 15)


def full_size(w):
    return N + (N // 2) * (w - 1)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def exp(ksa):
    """The experiments build in place of the product library for this module's engines (both bind the one HIP runtime)."""
    lib_mod = importlib.import_module("prgs-sdr-kspecanal_amd._lib")
    eng_mod = importlib.import_module("prgs-sdr-kspecanal_amd.engine")
    exp_lib = lib_mod.load(os.path.join(os.path.dirname(lib_mod.LIB_PATH), "libksa_exp.so"))   # missing: an error, not a skip
    saved = (lib_mod.lib, eng_mod.lib)
    lib_mod.lib = eng_mod.lib = exp_lib
    yield ksa
    lib_mod.lib, eng_mod.lib = saved
    for k in SWITCHES:
        os.environ.pop(k, None)


def set_env(**kw):
    for k in SWITCHES:
        os.environ.pop(k, None)
    for k, v in kw.items():
        if v is not None:
            os.environ[k] = str(v)


_C64 = {}


def samples_c64(w):
    """[NFRAMES][full_size(w)] complex64, computed once per W and never changed (callers copy before they edit)."""
    if w not in _C64:
        full = full_size(w)
        _C64[w] = orc.synth_iq(full * NFRAMES, 23 + w).astype(np.complex64).reshape(NFRAMES, full)
    return _C64[w]


def to_device(torch, ksa, x, fmt):
    """complex64 [frames][full] -> (device tensor of the format's I,Q pairs, format constant)"""
    if fmt == "c64":
        return torch.view_as_real(torch.from_numpy(np.ascontiguousarray(x))).cuda(), ksa.FMT_C64
    iq = np.stack([x.real, x.imag], axis=-1).reshape(x.shape[0], -1) * 0.7
    if fmt == "u8":
        return torch.from_numpy(orc.quantize_u8((x * 0.7).reshape(-1)).reshape(x.shape[0], -1)).cuda(), ksa.FMT_U8
    peak = float(np.max(np.abs(iq))) or 1.0
    if fmt == "s8":
        return torch.from_numpy(np.clip(np.rint(iq / peak * 127.0), -128, 127).astype(np.int8)).cuda(), ksa.FMT_S8
    return torch.from_numpy(np.clip(np.rint(iq / peak * 32767.0), -32768, 32767).astype(np.int16)).cuda(), ksa.FMT_S16


def run_once(ksa, torch, dev, fmt_id, w, fold, plain, split):
    set_env(KSA_PLAIN=1 if plain else None, KSA_NO_SPLIT=None if split else 1)
    eng = ksa.SpectrumEngine(N, full_size=full_size(w), non_overlap=0.5, window="hanning", cumu_mode=fold, xres=XRES,
                             max_frames=NFRAMES, stream=torch.cuda.current_stream().cuda_stream)
    db = torch.full((NFRAMES, eng.fft_size), -7.0, dtype=torch.float32, device="cuda")
    rows = torch.full((NFRAMES, eng.hm_width), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.frames_dev(dev, fmt_id, NFRAMES, cur_db=db, hm_rows=rows)
    torch.cuda.synchronize()
    st = eng.state()
    res = {"frames": st["frames"], "hm_index": st["hm_index"], "nwin": eng.num_windows}
    for k in ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg", "fftHM"):
        res[k] = st[k].view(np.uint64)           # float32 -> float64 is one-to-one on bit patterns, NaN payloads included
    res["cur_db"] = db.cpu().numpy()
    res["hm_rows"] = rows.cpu().numpy()
    eng.close()
    return res


def assert_same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray) and x.dtype == np.float32:
            assert np.array_equal(np.isnan(x), np.isnan(y)), "%s: %s has NaNs in other places" % (what, k)
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert np.array_equal(x, y), "%s: %s differs between the packed and the plain kernel" % (what, k)


def both(ksa, torch, x, fmt, w, fold, split=False):
    dev, fmt_id = to_device(torch, ksa, x, fmt)
    packed = run_once(ksa, torch, dev, fmt_id, w, fold, False, split)
    plain = run_once(ksa, torch, dev, fmt_id, w, fold, True, split)
    what = "W=%d %s %s%s" % (w, fold, fmt, " split" if split else "")
    assert packed["frames"] == NFRAMES and packed["nwin"] == w, what
    assert not np.any(packed["cur_db"] == np.float32(-7.0)), "%s: a frame's row was never written" % what
    assert_same_bits(packed, plain, what)
    return packed


@pytest.mark.parametrize("fmt", ["c64", "u8", "s8", "s16"])
@pytest.mark.parametrize("fold", ["AVG", "MAX", "MIN", "PSD"])
def test_packed_kernel_equals_plain_kernel(exp, torch_cuda, fold, fmt):
    for w in WINDOWS:
        r = both(exp, torch_cuda, samples_c64(w), fmt, w, fold)
        assert np.all(np.isfinite(r["cur_db"])), "W=%d %s %s: noise input gave a non-finite dB row" % (w, fold, fmt)


def test_window_split_shares(exp, torch_cuda):
    """Five frames on the default grid: every frame's windows are split over several workgroups (shares of one or two windows)."""
    for w in (4, 15):
        both(exp, torch_cuda, samples_c64(w), "c64", w, "AVG", split=True)


@pytest.mark.parametrize("fold", ["AVG", "MAX", "MIN", "PSD"])
def test_special_values(exp, torch_cuda, fold):
    """A NaN sample, +inf and -inf samples, an all-zero frame and denormal products, in windows of both parities."""
    for w in (4, 15):
        full = full_size(w)
        x = samples_c64(w).copy()
        x[0, 100] = complex(np.nan, 1.0)                   # first window only
        x[1, 2048 + 77] = complex(1.0, np.inf)             # windows 0 and 1
        x[1, full - 5] = complex(-np.inf, 0.0)             # last window
        x[2, :] = 0.0
        r = both(exp, torch_cuda, x, "c64", w, fold)
        assert np.all(np.isnan(r["cur_db"][0])), "a NaN sample must reach every bin"
        if fold != "MIN":       # (the MIN fold keeps the windows that do not hold the inf samples)
            assert not np.any(np.isfinite(r["cur_db"][1])), "an inf sample must reach every bin"
        assert np.all(np.isfinite(r["cur_db"][3])) and np.all(np.isfinite(r["cur_db"][4]))
        assert np.all(np.isneginf(r["cur_db"][2])), "an all-zero frame reads -inf dB (zeroSpan keeps it)"
        tiny = (samples_c64(w) * np.float32(1e-38)).astype(np.complex64)      # every tap product is a denormal
        assert np.any(tiny != 0)
        both(exp, torch_cuda, tiny, "c64", w, fold)
