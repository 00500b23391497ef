"""Ticket walk of spectrum_kernel: frames are handed to the persistent workgroups on demand -- the first unit of
a workgroup is blockIdx.x, every later one gridDim.x + a ticket from the engine's counter -- instead of by the stride gridDim.x.
A unit's dB row, waterfall row and ring slot are functions of its index alone, so both orders must give the SAME BITS.

Every case runs one input through the experiments build (libksa_exp.so, built beside the product library from the same sources;
only it reads environment switches) twice: in ticket order and with KSA_STATIC_WALK=1, the static walk.  KSA_GRID=5 holds the
grid at five workgroups and KSA_NO_SPLIT=1 keeps whole frames as units, so that a handful of frames draws tickets.  Compared,
as bit patterns (NaNs count): the per-frame dB rows, the waterfall rows, the ring with its index, Cur / Max / Min / Avg."""
import importlib
import os

import numpy as np
import pytest

import ksa_oracle as orc

pytestmark = pytest.mark.gpu

SWITCHES = ("KSA_STATIC_WALK", "KSA_GRID", "KSA_NO_SPLIT", "KSA_FS_SCRATCH_MB")


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


_IQ = {}


def iq_dev(torch, fmt, nframes, full, seed=7):
    """[nframes][full] samples on the device, complex64 as float pairs or uint8 I,Q; computed once per shape."""
    key = (fmt, nframes, full, seed)
    if key not in _IQ:
        x = orc.synth_iq(full * nframes, seed).astype(np.complex64).reshape(nframes, full)
        if fmt == "c64":
            _IQ[key] = torch.view_as_real(torch.from_numpy(x)).cuda()
        else:
            _IQ[key] = torch.from_numpy(orc.quantize_u8(x.reshape(-1) * 0.7).reshape(nframes, 2 * full)).cuda()
    return _IQ[key]


def alloc_outputs(torch, eng, batches):
    """dB rows and waterfall rows of every batch, filled with a sentinel; the fills run on torch's stream, so they are waited for
    here, before anything is enqueued on an engine's stream."""
    outs = [(torch.full((nf, eng.fft_size), -7.0, dtype=torch.float32, device="cuda"),
             torch.full((nf, eng.hm_width), -7.0, dtype=torch.float32, device="cuda")) for _, nf in batches]
    torch.cuda.synchronize()
    return outs


def run_batches(ksa, eng, dev, fmt, batches, outs):
    """Enqueue `batches` = [(first frame, frames)] on the engine without a synchronise in between."""
    for (f0, nf), (db, rows) in zip(batches, outs):
        eng.frames_dev(dev[f0:f0 + nf], ksa.FMT_C64 if fmt == "c64" else ksa.FMT_U8, nf, cur_db=db, hm_rows=rows)
    return outs


def collect(torch, eng, outs):
    torch.cuda.synchronize()
    st = eng.state()
    res = {"frames": st["frames"], "hm_index": st["hm_index"]}
    for k in ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg", "fftHM"):
        res[k] = st[k].view(np.uint64)           # float32 -> float64 is one-to-one on bit patterns, NaN payloads included
    for i, (db, rows) in enumerate(outs):
        res["db%d" % i] = db.cpu().numpy().view(np.uint32)
        res["rows%d" % i] = rows.cpu().numpy().view(np.uint32)
    return res


def assert_same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), "%s: %s differs between the ticket walk and the static walk" % (what, k)


def both_orders(ksa, torch, n, full, q, fmt, batches, env, window="hanning"):
    """The same batches through a fresh engine per order; returns (tickets, static)."""
    total = max(f0 + nf for f0, nf in batches)
    dev = iq_dev(torch, fmt, total, full)
    res = []
    for static in (None, 1):
        set_env(KSA_STATIC_WALK=static, **env)
        eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window=window, max_frames=max(nf for _, nf in batches),
                                 stream=torch.cuda.current_stream().cuda_stream)
        res.append(collect(torch, eng, run_batches(ksa, eng, dev, fmt, batches, alloc_outputs(torch, eng, batches))))
        eng.close()
    return res


GRID5 = {"KSA_GRID": 5, "KSA_NO_SPLIT": 1}


# nframes: below the grid (no ticket drawn), equal to it, one more, and not a multiple of it.
# q: 0.5 / 0.25 are the sample-reuse kernels RM = 8 / RM = 4, 0.1 the general path RM = 0.
@pytest.mark.parametrize("fmt", ["c64", "u8"])
@pytest.mark.parametrize("q", [0.5, 0.25, 0.1])
def test_n4096_ticket_walk_equals_static_walk(exp, torch_cuda, q, fmt):
    n, full = 4096, 32768
    for nframes in (3, 5, 6, 23):
        t, s = both_orders(exp, torch_cuda, n, full, q, fmt, [(0, nframes)], GRID5)
        assert t["frames"] == nframes
        assert_same_bits(t, s, "N=4096 q=%s %s nframes=%d" % (q, fmt, nframes))
        assert not np.any(t["db0"] == np.float32(-7.0).view(np.uint32)), "a frame's row was never written"


def test_window_split_units(exp, torch_cuda):
    """Two frames on the default grid: the units are (frame, part) and combine_parts_kernel follows.  Then a frame long enough
    that the (frame, part) shares draw tickets on five workgroups (1281 windows over 256 parts: five windows per unit)."""
    t, s = both_orders(exp, torch_cuda, 4096, 32768, 0.5, "c64", [(0, 2)], {})
    assert_same_bits(t, s, "window split, default grid")
    t, s = both_orders(exp, torch_cuda, 4096, 4096 + 2048 * 1280, 0.5, "c64", [(0, 3)], {"KSA_GRID": 5})
    assert_same_bits(t, s, "window split, five workgroups")


def test_n64_runs_of_frames_per_ticket(exp, torch_cuda):
    """N = 64.  complex64 runs spectrum64_kernel (single-wave workgroups): a ticket hands out a run of consecutive frames (five at
    71 windows per frame), and only batches of at least two runs per workgroup draw tickets -- 23 frames on five workgroups keep
    the stride walk, 50 is the threshold, 53 and 117 end in a short run.  uint8 input runs spectrum_kernel<64> with several
    transforms per workgroup (S > 1): those instances walk by stride whatever the switch says."""
    for nframes in (23, 50, 53, 117):
        t, s = both_orders(exp, torch_cuda, 64, 512, 0.1, "c64", [(0, nframes)], GRID5, window="ones")
        assert t["frames"] == nframes
        assert_same_bits(t, s, "N=64 c64 nframes=%d" % nframes)
        assert not np.any(t["db0"] == np.float32(-7.0).view(np.uint32)), "a frame's row was never written"
    t, s = both_orders(exp, torch_cuda, 64, 512, 0.1, "c64", [(0, 117)], GRID5, window="hanning")     # the generic (tap-reading) form
    assert_same_bits(t, s, "N=64 c64 hanning")
    t, s = both_orders(exp, torch_cuda, 64, 512, 0.1, "u8", [(0, 23)], GRID5, window="ones")
    assert_same_bits(t, s, "N=64 u8")


def test_n1024_pair_kernel_runs_of_pairs_per_ticket(exp, torch_cuda, ksa):
    """N = 1024 at a batch large enough for spectrum_pair_kernel (two frames per workgroup; from 2 x the resident workgroups on):
    units are pairs, four per ticket at three windows per frame; the odd batch ends in a half pair and a short run."""
    probe = ksa.SpectrumEngine(1024, full_size=2048, non_overlap=0.5, window="hanning", max_frames=4)
    info = probe.kernel_info()
    probe.close()
    assert info["path"] == 4, "N = 1024 no longer has the pair kernel"
    nframes = 2 * info["grid"] + 3        # the switch-over is at two frames per resident workgroup of the pair kernel (4096 + 3)
    t, s = both_orders(exp, torch_cuda, 1024, 2048, 0.5, "c64", [(0, nframes)], {"KSA_GRID": 5})
    assert t["frames"] == nframes
    assert_same_bits(t, s, "N=1024 pairs")
    assert not np.any(t["db0"] == np.float32(-7.0).view(np.uint32)), "a frame's row was never written"


def test_n65536_resets_the_counter_for_every_chunk(exp, torch_cuda):
    """Path 2: the 4096-point kernel is the second stage, launched once per chunk of first-stage scratch (one frame per chunk
    here: three launches, 16 sub-frames of 7 windows each on five workgroups), the counter zeroed in front of each."""
    env = dict(GRID5, KSA_FS_SCRATCH_MB=4)
    t, s = both_orders(exp, torch_cuda, 65536, 4 * 65536, 0.5, "c64", [(0, 3)], env)
    assert t["frames"] == 3
    assert_same_bits(t, s, "N=65536")


def test_two_batches_without_a_synchronise(exp, torch_cuda):
    """The second batch's counter reset is ordered behind the first batch's kernel on the engine's stream."""
    t, s = both_orders(exp, torch_cuda, 4096, 32768, 0.5, "c64", [(0, 23), (23, 17)], GRID5)
    assert t["frames"] == 40
    assert_same_bits(t, s, "two batches")


def test_two_engines_on_two_streams_have_their_own_counters(exp, torch_cuda):
    ksa, torch = exp, torch_cuda
    n, full, nframes = 4096, 32768, 23
    devs = [iq_dev(torch, "c64", nframes, full, seed=11 + i) for i in range(2)]
    res = []
    for static in (None, 1):
        set_env(KSA_STATIC_WALK=static, **GRID5)
        streams = [torch.cuda.Stream() for _ in range(2)]
        torch.cuda.synchronize()
        engs = [ksa.SpectrumEngine(n, full_size=full, non_overlap=0.5, window="hanning", max_frames=nframes, stream=st.cuda_stream)
                for st in streams]
        batches = [(0, nframes)] * 2
        outs = [alloc_outputs(torch, eng, batches) for eng in engs]
        for rep in range(2):         # enqueued back to back: a, b, a, b
            for eng, dev, o in zip(engs, devs, outs):
                run_batches(ksa, eng, dev, "c64", batches[rep:rep + 1], o[rep:rep + 1])
        res.append([collect(torch, eng, outs[i]) for i, eng in enumerate(engs)])
        for eng in engs:
            eng.close()
    for i in range(2):
        assert res[0][i]["frames"] == 2 * nframes
        assert_same_bits(res[0][i], res[1][i], "engine %d of two" % i)
    assert not np.array_equal(res[0][0]["db0"], res[0][1]["db0"])     # different inputs
