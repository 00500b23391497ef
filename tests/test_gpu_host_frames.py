"""GPU tests of the batched zeroSpan from host memory (ksa_frames_c64 / _u8, ABI 5): bit for bit the state of ksa_frames_dev on a
device copy of the same batch for every plan the library picks (8 x 8, pair kernel, window split, first stage), slot boundaries
crossed on purpose; the commit = 0 merge; the reference oracle and INTEGRATION.md run verbatim; refusals; the front end's
frameBatch end to end; a plain C client."""
import ctypes as C
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import ksa_oracle as orc
from conftest import golden, load_pkg, ROOT
from test_gpu_parity import assert_db, GAIN
from test_host_cli import integration_blocks

pytestmark = pytest.mark.gpu
CURVES = ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg")
SLOT_BYTES = 32 << 20          # include/ksa.h KSA_FRAME_SLOT_BYTES


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def slot_frames(frame_bytes):
    """include/ksa.h: KSA_FRAME_SLOT_BYTES rounded down to a multiple of 4 whole blocks, at least 4."""
    return max(4, SLOT_BYTES // frame_bytes // 4 * 4)


def _digest(a):
    return hashlib.sha1(memoryview(np.ascontiguousarray(a)).cast("B")).hexdigest()


def _same_state(a, b, what):
    for k in CURVES + ("fftHM",):
        assert np.array_equal(a[k], b[k], equal_nan=True), "%s: %s differs" % (what, k)
    assert a["hm_index"] == b["hm_index"] and a["frames"] == b["frames"], (what, a["hm_index"], b["hm_index"], a["frames"], b["frames"])


def _blocks(fmt, frames, full, seed):
    rng = np.random.default_rng(seed)
    if fmt == "u8":
        return rng.integers(0, 256, (frames, 2 * full), dtype=np.uint8)
    x = rng.standard_normal((frames, 2 * full), dtype=np.float32) * np.float32(0.3)
    return x.view(np.complex64)


def _dev_run(torch, ksa, eng, blocks, first=0, total=None, commit=True):
    """ksa_frames_dev on a torch copy of `blocks`; returns (cur_db, hm_rows) on the host."""
    k = blocks.shape[0]
    fmt = ksa.FMT_U8 if blocks.dtype == np.uint8 else ksa.FMT_C64
    src = torch.from_numpy(blocks) if fmt == ksa.FMT_U8 else torch.view_as_real(torch.from_numpy(blocks))
    iq = src.to("cuda")
    db = torch.empty((k, eng.fft_size), dtype=torch.float32, device="cuda")
    rows = torch.empty((k, eng.hm_width), dtype=torch.float32, device="cuda")
    eng.frames_dev(iq, fmt, k, first_index=first, total_frames=total, cur_db=db, hm_rows=rows, commit=commit)
    eng.synchronize()
    return db.cpu().numpy(), rows.cpu().numpy()


# (fft_size, full_size, nonOverlap, window): N = 64 runs the 8 x 8 plan (rectangular: the tap-free kernel), N = 1024 the pair
# kernel on large batches, N = 16384 the 32-point plan, N = 65536 the radix-16 first stage in chunks
CASES = [(64, 512, 0.1, "hanning"), (64, 512, 0.1, "ones"), (512, 4096, 0.5, "hanning"), (1024, 8192, 0.5, "hanning"),
         (4096, 32768, 0.5, "hanning"), (16384, 131072, 0.1, "hanning"), (65536, 524288, 0.25, "hanning")]


@pytest.mark.parametrize("fold", ["AVG", "MAX"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_%s" % (c[0], c[3]))
def test_host_batch_equals_device_batch_bit_for_bit(ksa, torch_cuda, case, fold):
    """ksa_frames_c64 / _u8 from pageable and from pinned memory against ksa_frames_dev on a device copy of the same array:
    every curve, the ring, hm_index, frames_seen and both per-frame outputs, for a batch over >= 3 slots whose last slot holds
    an odd number of blocks, then a small batch (3 blocks: the window-split plan from N = 1024 up) on the same engines.  The
    caller's buffer is left as it was."""
    torch = torch_cuda
    n, full, q, win = case
    for fmt in ("c64", "u8"):
        frame_bytes = full * (2 if fmt == "u8" else 8)
        sf = slot_frames(frame_bytes)
        big = 3 * sf + 5
        if n == 1024:                 # large enough for the two-frames-per-workgroup kernel (chosen from 2 x its grid up)
            probe = ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window=win)
            info = probe.kernel_info()
            probe.close()
            assert info["path"] == 4
            big = max(big, 2 * info["grid"] + 5)
        if (big % sf) % 2 == 0:
            big += 1
        assert big > 2 * sf and (big % sf) % 2 == 1
        x_big, x_small = _blocks(fmt, big, full, n + big), _blocks(fmt, 3, full, n + 3)
        mk = lambda: ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window=win, cumu_mode=fold, gain=GAIN, xres=512,
                                        max_frames=big)
        ref = mk()
        want = [_dev_run(torch, ksa, ref, x_big)]
        st_big = ref.state()
        want.append(_dev_run(torch, ksa, ref, x_small))
        st_small = ref.state()
        ref.close()
        for kind in ("pageable", "pinned"):
            bufs = []
            for x in (x_big, x_small):
                if kind == "pinned":
                    pb = ksa.PinnedBuffer(x.shape, x.dtype)
                    pb.array[...] = x
                    bufs.append(pb)
                else:
                    bufs.append(x)
            arrays = [b.array if kind == "pinned" else b for b in bufs]
            before = [_digest(a) for a in arrays]
            eng = mk()
            what = "N=%d %s %s %s %s" % (n, win, fold, fmt, kind)
            got = eng.frames(arrays[0], cur_db=True, hm_rows=True)
            _same_state(eng.state(), st_big, what + " big batch")
            for g, w, name in zip(got, want[0], ("cur_db", "hm_rows")):
                assert np.array_equal(g, w, equal_nan=True), "%s big batch: %s differs" % (what, name)
            got = eng.frames(arrays[1], cur_db=True, hm_rows=True)
            _same_state(eng.state(), st_small, what + " small batch")
            for g, w, name in zip(got, want[1], ("cur_db", "hm_rows")):
                assert np.array_equal(g, w, equal_nan=True), "%s small batch: %s differs" % (what, name)
            assert [_digest(a) for a in arrays] == before, what + ": the input buffer changed"
            eng.close()
            for b in bufs:
                if kind == "pinned":
                    b.close()


def test_commit0_halves_merge_like_the_device_entry(ksa, torch_cuda):
    """Two engines on device 0 each take half of a run through the host entry with commit = 0 (exchange blocks equal to the device
    entry's), then ksa_allreduce_state merges them: both handles equal the same split done with ksa_frames_dev."""
    torch = torch_cuda
    n, full, q, half = 4096, 32768, 0.5, 300
    x = _blocks("c64", 2 * half, full, 5150)
    mk = lambda: ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window="hanning", gain=GAIN, xres=512, max_frames=half)
    hosts, devs = [mk(), mk()], [mk(), mk()]
    for r in range(2):
        part = x[r * half:(r + 1) * half]
        for e in (hosts[r], devs[r]):
            e.set_hm_index((r * half) % 128)
        hosts[r].frames(part, first_index=r * half, total_frames=2 * half, commit=False)
        _dev_run(torch, ksa, devs[r], part, first=r * half, total=2 * half, commit=False)
        a = torch.as_tensor(hosts[r].exchange(), device="cuda").cpu().numpy()
        b = torch.as_tensor(devs[r].exchange(), device="cuda").cpu().numpy()
        assert np.array_equal(a, b, equal_nan=True), "exchange block of rank %d" % r
    ksa.allreduce_state(hosts, half)
    ksa.allreduce_state(devs, half)
    for r in range(2):
        _same_state(hosts[r].state(), devs[r].state(), "merged rank %d" % r)
    _same_state(hosts[0].state(), hosts[1].state(), "host ranks")
    assert hosts[0].state()["frames"] == 2 * half
    for e in hosts + devs:
        e.close()


def test_host_batch_against_the_oracle(ksa, torch_cuda):
    """300 frames in one ksa_frames_c64 call and in one ksa_frames_u8 call against the reference's sequential frame loop
    (K:464-484): curves, per-frame dB rows, per-frame waterfall rows and the ring."""
    n, full, q, frames = 1024, 8192, 0.5, 300
    x = (orc.synth_iq(full * frames, 4711) * 0.6).astype(np.complex64).reshape(frames, full)
    raw = orc.quantize_u8(x.reshape(-1)).reshape(frames, 2 * full)
    for blocks, ref_in in ((x, x), (raw, orc.unpack_u8(raw.reshape(-1)).reshape(frames, full))):
        st, db_ref, _ = orc.zerospan_batch(ref_in, n, q, orc.window_table("kaiser", n), "AVG", GAIN, 256)
        eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window="kaiser", gain=GAIN, xres=256, max_frames=frames)
        db, rows = eng.frames(blocks, cur_db=True, hm_rows=True)
        got = eng.state()
        what = "oracle %s" % blocks.dtype
        for k in CURVES:
            assert_db(got[k], getattr(st, k[4:].lower()), what="%s %s" % (what, k))
        assert_db(db, db_ref, what=what + " per-frame dB")
        assert_db(rows, np.array([orc.plotcompress(r, 256, "MAX") for r in db_ref]), what=what + " rows")
        assert_db(got["fftHM"], st.hm, what=what + " ring")
        assert got["hm_index"] == frames % 128 and got["frames"] == frames
        eng.close()


class _Quit(Exception):
    pass


@pytest.mark.parametrize("tag", ["n4096", "hm_n512"])
def test_integration_section3_batch_block_runs_verbatim(ksa, torch_cuda, tag):
    """INTEGRATION.md section 2 (ksa_open with ksaMaxFrames) and section 3's second block -- every golden frame handed over in ONE
    ksa_frames_c64 call -- executed as they stand against the reference's own zeroSpan runs."""
    g = golden("zerospan_" + tag)
    n, full, q, frames = int(g["fft_size"]), int(g["full"]), float(g["non_overlap"]), int(g["frames"])
    x = g["iq"].reshape(frames, full)
    blocks = integration_blocks()
    open_src = blocks["2"][0].replace('C.CDLL("libksa.so")', "C.CDLL(%r)" % ksa.LIB_PATH)
    xres = int(g["xres"])
    d = {"fftSize": n, "fullSize": full, "curScanNonOverlap": q, "curScanCumuMode": "AVG",
         "theWin": orc.window_table(str(g["window"]), n), "gain": float(g["gain"]), "minAmp4Clip": (1 / 256) * 1e-5, "xRes": xres,
         "sdr": object(), "bDataMax": True, "bDataMin": True, "bDataAvg": True, "PltHeatMapWidth": min(n, xres),
         "ksaMaxFrames": frames}
    feed = iter(list(x))

    def sdr_read(sdr, length):
        b = next(feed)
        assert len(b) == length
        return b.astype(np.complex128)

    def prg_quit(dd, msg):
        raise _Quit(msg)

    ns = {"sdr_read": sdr_read, "prg_quit": prg_quit, "gD": d, "d": d, "__name__": "kspecanal_patch"}
    exec(compile(open_src, "INTEGRATION.md#2", "exec"), ns)
    exec(compile(blocks["3"][1], "INTEGRATION.md#3b", "exec"), ns)
    for k in CURVES:
        assert_db(d[k], g[k.replace("Fft.", "").lower()], what="INTEGRATION section 3 batch " + k)
    assert ns["indexHM"] == frames % 128 and ns["seen"].value == frames
    if "hm" in g.files:
        assert_db(ns["fftHM"][:frames], g["hm"][:frames], what="INTEGRATION section 3 batch waterfall")
    ns["ksa"].ksa_destroy(d["ksa"])


def test_refusals_leave_the_state_alone(ksa, torch_cuda):
    """nframes 0 or above max_frames, a batch outside [0, total_frames) and a null pointer are refused before anything is
    enqueued: the error text is set and read_state / frames_seen stay as they were."""
    n, full = 1024, 8192
    eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=0.5, window="hanning", gain=GAIN, xres=256, max_frames=8)
    x = _blocks("c64", 8, full, 99)
    eng.frames(x[:5])
    before = eng.state()
    lib, h = ksa.lib, eng._h
    p = x.ctypes.data_as(C.c_void_p)
    for args, word in (((p, 0, 0, 0), b"nframes"), ((p, 9, 0, 9), b"nframes"), ((p, 4, -1, 4), b"outside"),
                       ((p, 4, 2, 5), b"outside"), ((None, 4, 0, 4), b"null")):
        for fn in (lib.ksa_frames_c64, lib.ksa_frames_u8):
            lib.ksa_merge_gathered_dev(h, p, 0, 1, 0)      # leaves "world 0 < 1" behind: each refusal must write its own text
            rc = fn(h, *args, None, None, 1)
            err = lib.ksa_last_error()
            assert rc != 0 and word in err, (args, err)
            _same_state(eng.state(), before, "after refused %s" % (args[1:],))
    eng.close()


# ------------------------------------------------------------------------------------------------ the front end
def _capture(tmp_path, frames, full, seed):
    x = orc.synth_iq(16 * 1024 + full * frames, seed) * 0.7
    raw = orc.quantize_u8(x)
    path = tmp_path / ("capture%d.bin" % seed)
    raw.tofile(path)
    blocks = orc.unpack_u8(raw[2 * 16 * 1024:]).reshape(frames, full)       # sdr_setup discards 16Ki first (K:301)
    return str(path), blocks


def _run(K, orig, monkeypatch, capsys, argv):
    seen = {}

    def spy(d, eng, scan=False):
        seen["host_hm"] = np.array(d["fftHM"])           # the host copy the per-batch hand-offs assembled
        st = orig(d, eng, scan)
        seen["state"] = st
        return st

    monkeypatch.setattr(K, "_materialize", spy)
    capsys.readouterr()
    d = K.main(argv)
    out = capsys.readouterr().out
    return d, seen, len(re.findall(r"^ZeroSpan:\d+:", out, flags=re.M))


def test_front_end_frame_batch_end_to_end(ksa, torch_cuda, tmp_path, monkeypatch, capsys):
    """`frameBatch 64 prgLoopCnt 300` over a uint8 `file:` capture, complex64 and uint8 hand-over: the curves match the oracle,
    fftHMIndex is 300 % 128, the host waterfall assembled batch by batch equals the device ring, five progress lines; a capture
    shorter than prgLoopCnt processes the same frames as frameBatch 1."""
    load_pkg()
    K = __import__("importlib").import_module("prgs-sdr-kspecanal_amd.kspecanal")
    orig = K._materialize
    n, frames = 4096, 300
    full = orc.full_size(n, 2.4e6)
    path, blocks = _capture(tmp_path, frames, full, 808)
    st, _, _ = orc.zerospan_batch(blocks, n, 0.5, orc.window_table("hanning", n), "AVG", 19.1, 512)
    common = ["zeroSpan", "fftSize", str(n), "window", "hanning", "curScanNonOverlap", "0.5", "bPltLevels", "false",
              "bPltHeatMap", "false", "source", "file:%s" % path]
    for fmt in ("c64", "u8"):
        d, seen, lines = _run(K, orig, monkeypatch, capsys, common + ["prgLoopCnt", str(frames), "frameBatch", "64", "iqFormat", fmt])
        for k in ("Cur", "Max", "Min", "Avg"):
            assert_db(d["Fft." + k], getattr(st, k.lower()), what="frameBatch %s %s" % (fmt, k))
        assert d["fftHMIndex"] == frames % 128 and seen["state"]["frames"] == frames
        assert np.array_equal(seen["host_hm"], seen["state"]["fftHM"]), "host waterfall differs from the device ring"
        assert lines == 5, lines
    # a capture shorter than prgLoopCnt: the same frames as frameBatch 1, then the run stops
    path2, _ = _capture(tmp_path, 70, full, 909)
    short = [a if a != "file:%s" % path else "file:%s" % path2 for a in common] + ["prgLoopCnt", str(frames), "iqFormat", "u8"]
    d1, seen1, _ = _run(K, orig, monkeypatch, capsys, short + ["frameBatch", "1"])
    d64, seen64, lines = _run(K, orig, monkeypatch, capsys, short + ["frameBatch", "64"])
    assert seen1["state"]["frames"] == seen64["state"]["frames"] == 70 and d64["cmd.stop"] is True and lines == 2
    for k in CURVES:                 # (not bit for bit: a batch picks another window-split plan than single blocks)
        assert_db(d64[k], d1[k], what="short capture " + k)


def test_plain_c_client_batch(tmp_path):
    """tests/c_client/ksa_client_frames.c (C99): 256 blocks from ksa_host_alloc memory through one ksa_frames_c64 call; the tone
    bin is the Max peak at its closed-form level and the ring is back at row 0."""
    exe = str(tmp_path / "ksa_client_frames")
    pkg = os.path.join(ROOT, "prgs-sdr-kspecanal_amd")
    rocm = "/opt/rocm/lib"
    r = subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "c_client", "ksa_client_frames.c"), "-o", exe, "-L", pkg, "-lksa", "-lm",
                        "-Wl,-rpath," + pkg, "-Wl,-rpath," + rocm, "-Wl,-rpath-link," + rocm], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "c frames client ok" in r.stdout
