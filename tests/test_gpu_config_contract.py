"""GPU tests of the library on caller-chosen geometry: window starts in any order and at any spacing, any tap table, any scale
(include/ksa.h: "the caller chooses segmentation and scale") -- against the float64 model of config_model.py, which is written from
the header's formulas and knows nothing of the three start generators of engine.py.

Which kernel serves an engine is decided by the SHAPE of its starts (ksa_api.hip): choose_plan picks the sample-reuse kernels
(RM 8 / RM 4) when every hop is the same and equals N/2 or N/4, and those compute start0 + k*RM*L instead of reading the list;
RAW transforms the window listed last; the AVG weights follow the list position; the window split hands runs of list positions to
different workgroups; launch_pfb takes the ring form only for starts[k] == k*N.  The cases below are chosen from those rules and
each docstring cites the one it sits on; kernel_info()["path"] is asserted as in the path tables of the other GPU files.

Tolerances are the project's own, imported as they stand: assert_lin (1e-5 of the strongest bin), assert_db, assert_psd."""
import numpy as np
import pytest

import config_helper as ch
import config_model as cm
import ksa_oracle as orc
from test_gpu_parity import assert_lin, assert_db
from test_gpu_pfb import _dev, _quantized, _xres
from test_gpu_psd import assert_psd

pytestmark = pytest.mark.gpu

SCALE = 0.0123                    # no generator produces it (2*winAdj/N, 1/(Fs*sum(w^2)*K), 2/sum(taps))
GAIN, U8_OFFSET, U8_SCALE = 7.25, 127.0, 128.0          # not the defaults (19.1, 127.5, 127.5)
MODE = {"RAW": cm.RAW, "AVG": cm.AVG, "MAX": cm.MAX, "MIN": cm.MIN, "PSD": cm.PSD}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


_SRC = []


def _take(total, off=0):
    """`total` samples of ONE draw of the oracle's synthetic IQ (2^20 samples, made once and left unchanged), from `off`."""
    if not _SRC:
        _SRC.append((orc.synth_iq(1 << 20, 20260) * 0.7).astype(np.complex64))
    assert off + total <= len(_SRC[0])
    return _SRC[0][off:off + total]


def _taps(n, segments=1, seed=0):
    """A seeded random tap table, float32-exact, with negative values and exact zeros; from three segments up the second one is
    all zero."""
    t = np.random.default_rng(77 + seed + n).standard_normal(segments * n).astype(np.float32)
    t[::7] = 0.0
    if segments >= 3:
        t[n:2 * n] = 0.0
    assert np.any(t < 0) and np.any(t == 0)
    return t.astype(np.float64)


def _fmts(ksa):
    return {"c64": ksa.FMT_C64, "u8": ksa.FMT_U8, "s8": ksa.FMT_S8, "s16": ksa.FMT_S16}


def _block(src, fmt_name, first, count):
    """Samples [first, first + count) of the array handed to the device, as the model's complex128."""
    if fmt_name == "c64":
        return cm.unpack(src[first:first + count], cm.C64)
    code = {"u8": cm.U8, "s8": cm.S8, "s16": cm.S16}[fmt_name]
    return cm.unpack(src[2 * first:2 * (first + count)], code, U8_OFFSET, U8_SCALE)


# ---- the geometry families ----------------------------------------------------------------------------------------------------
def geometry(n, w, fam):
    """(starts int32[...], full_size) of family `fam` with `w` windows at fft_size n: every start inside full_size."""
    k = np.arange(w, dtype=np.int64)
    a = 3 + k * (n // 2)
    if fam == "a":          # uniform hop N/2 from an odd start0: reuse RM 8
        s = a
    elif fam == "b":        # uniform hop N/4 from start0 = 5: reuse RM 4
        s = 5 + k * (n // 4)
    elif fam == "c":        # hop N/2 everywhere but the last: the general path right next to the rule
        s = a.copy()
        s[-1] += 7
    elif fam == "d":        # two windows at hop N/2: the `same` loop of choose_plan never runs
        s = a[:2]
    elif fam == "e":        # (a) reversed: hop -N/2, general path; RAW = the window listed last, AVG weights by list position
        s = a[::-1]
    elif fam == "f":        # shuffled, one start listed twice (hop 0), starts of both parities
        rng = np.random.default_rng(1000 * n + w)
        s = k * (n // 2) + rng.integers(0, n // 4, w)
        s[0], s[1] = s[0] | 1, s[1] & ~1
        s = np.append(s, s[1])
        rng.shuffle(s)
    elif fam == "g34":      # uniform, but not a reuse hop: 3N/4
        s = 1 + k * (3 * n // 4)
    elif fam == "g8":       # uniform, but not a reuse hop: N/8
        s = 2 + k * (n // 8)
    elif fam == "h":        # one window that ends with the block, full_size no multiple of 4: the last sample of the descriptor's range
        return np.array([n + 3], dtype=np.int32), 2 * n + 3
    else:
        raise ValueError(fam)
    full = int(s.max()) + n + 5
    assert s.min() >= 0 and (fam != "f" or set(s % 2) == {0, 1})
    return s.astype(np.int32), full


# the folds a family changes the answer of (e and f are order sensitive: AVG and RAW always)
FOLDS = {"a": ("AVG", "MAX", "MIN", "RAW", "PSD"), "b": ("AVG", "MIN", "PSD"), "c": ("AVG", "MAX"), "d": ("AVG", "RAW", "PSD"),
         "e": ("AVG", "RAW", "MAX"), "f": ("AVG", "RAW", "MIN", "PSD"), "g34": ("AVG", "MAX"), "g8": ("AVG", "PSD"),
         "h": ("RAW", "AVG", "PSD")}
ALL = ("a", "b", "c", "d", "e", "f", "g34", "g8", "h")
# N: (path of kernel_info, windows, families, batches)
# batches: an int = frames at stride fullSize; "split" = 3 frames (N >= 1024: window split); "fill" = grid//2 + 3 frames at stride
# 512; "below" = 2*grid - 1 frames at stride 64 (N = 1024: the largest batch the one-frame kernel serves, unsplit as long as it
# holds fewer than four times the pair kernel's workgroups); "pair" = 2*grid + 1 frames at stride 64 (pair kernel, half pair last)
SIZES = {
    16: (0, (5,), ALL, (3,)),                                     # one transform pass (M = 1)
    64: (5, (17, 33), ALL, (3,)),                                 # 8 x 8 plan (complex64), spectrum_kernel<64> (integers); rounds of 16 plus one
    256: (0, (7,), ALL, (5,)),                                    # several transforms per workgroup (S > 1), 7 windows: a ragged last round
    1024: (4, (7,), ALL, ("split", "fill", "below", "pair")),
    4096: (0, (5,), ("a", "c", "d", "e"), (1, "fill")),           # 1 frame: split, shares of one window skip the ping-pong loop's second half
    8192: (3, (4,), ("a", "e", "f", "h"), (2,)),                  # 32 points per thread
    32768: (2, (3,), ("a", "f", "h"), (3,)),                      # radix-16 first stage: both alignment branches (starts and frame bases of both parities)
    240: (6, (5,), ALL, (3,)),                                    # mixed radix
    1000: (6, (5,), ALL, (3,)),
}
CASES = [(n, w, fam, b) for n, (_, ws, fams, batches) in SIZES.items() for w in ws for fam in fams for b in batches]
INT_FMTS = ("u8", "s8", "s16")


def _batch(batch, grid, full):
    """(frames, stride)."""
    if batch == "split":
        return 3, full
    if batch == "fill":
        return grid // 2 + 3, 512
    if batch == "below":
        return 2 * grid - 1, 64
    if batch == "pair":
        return 2 * grid + 1, 64
    return int(batch), full


def _engine(ksa, n, starts, full, taps, fold, frames, min_amp=0.0):
    eng = ksa.SpectrumEngine(n, full_size=full, window=taps, cumu_mode=fold, starts=starts, mag_scale=SCALE, gain=GAIN, min_amp=min_amp,
                             xres=_xres(n), max_frames=frames, u8_offset=U8_OFFSET, u8_scale=U8_SCALE)
    assert eng.num_windows == len(starts) and np.array_equal(eng._starts32, starts) and eng.mag_scale == SCALE and eng.full_size == full
    return eng


_GRID = {}


def _grid(ksa, n):
    """kernel_info()["grid"] of an engine at n (N = 1024: the pair kernel's) and the path check of the size."""
    if n not in _GRID:
        starts, full = geometry(n, 3, "a")
        probe = _engine(ksa, n, starts, full, _taps(n), "AVG", 1)
        info = probe.kernel_info()
        probe.close()
        assert info["path"] == SIZES[n][0], info
        _GRID[n] = info["grid"]
    return _GRID[n]


@pytest.mark.parametrize("case", CASES, ids=["%d-w%d-%s-%s" % c for c in CASES])
def test_folds_on_caller_chosen_starts(ksa, torch_cuda, case):
    """Every family of starts at every size and batch shape, complex64 and one integer format (rotating), linear output, every
    fold the family changes the answer of -- against the header's formulas.

    choose_plan: `hop = starts[1] - starts[0]`, all hops equal, hop == N/2 or N/4, N >= 1024, path 0 -> reuse_m; spectrum_kernel
    then forms start0 + k*RM*L (a, b: start0 odd / 5; d: the loop over i >= 2 is empty).  c, e, f, g miss the rule by one hop, the
    sign, the order and the hop length: p.starts[k] is read.  run_transform: RAW -> d_start_last, one window (e, f: it must be the
    one LISTED last).  ksa_window_body.inc: the AVG weight 2^-(nwin-k) by list position k.  launch_split: `plan*2 <= capacity`
    splits the list into contiguous shares (3 frames at N >= 1024, 1 frame at 4096); launch_spec_t: >= 2 x grid frames take the
    pair kernel at N = 1024.  h: the window's last sample is the last one the frame's buffer descriptor covers."""
    torch = torch_cuda
    n, w, fam, batch = case
    grid = _grid(ksa, n)
    starts, full = geometry(n, w, fam)
    frames, stride = _batch(batch, grid, full)
    taps = _taps(n)
    int_name = INT_FMTS[CASES.index(case) % 3]
    x = _take((frames - 1) * stride + full, off=CASES.index(case) % 11)
    srcs = (("c64", x), (int_name, _quantized(ksa, x, _fmts(ksa)[int_name])))
    devs = {name: _dev(torch, src) for name, src in srcs}
    out = torch.empty((frames, n), dtype=torch.float32, device="cuda")
    check = sorted(set(np.linspace(0, frames - 1, min(frames, 5)).astype(int)))
    for fold in FOLDS[fam]:
        eng = _engine(ksa, n, starts, full, taps, fold, frames)
        assert eng.kernel_info()["path"] == SIZES[n][0]
        for name, src in srcs:
            out.fill_(-1.0)
            eng.curscan_dev(devs[name], _fmts(ksa)[name], frames, out, frame_stride=stride)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert np.all(got >= 0), "%s %s: a frame was not written" % (fold, name)
            for f in check:
                want = cm.spectrum(_block(src, name, f * stride, full), n, starts, taps, SCALE, MODE[fold])
                what = "N=%d %s %s %s frame %d/%d starts %s" % (n, fam, fold, name, f, frames, starts[:6])
                (assert_psd if fold == "PSD" else assert_lin)(got[f], want, what=what)
        eng.close()


@pytest.mark.parametrize("n", sorted(SIZES))
def test_db_modes_with_their_own_gain_and_clip_level(ksa, torch_cuda, n):
    """One case per size through KSA_OUT_DB and KSA_OUT_DB_CLIP with gain 7.25 and a min_amp inside the range of the bins (the
    median of the linear spectrum): LogNoGain / Clip2MinAmp of the header on family f (family a at the sizes that do not list f:
    4096), AVG and PSD."""
    torch = torch_cuda
    fam = "f" if "f" in SIZES[n][2] else "a"
    starts, full = geometry(n, SIZES[n][1][0], fam)
    taps, frames = _taps(n), 2
    x = _take(frames * full, off=n % 13)
    dev = _dev(torch, x)
    out = torch.empty((frames, n), dtype=torch.float32, device="cuda")
    for fold, check in (("AVG", assert_lin), ("PSD", assert_psd)):
        lin = [cm.spectrum(x[f * full:(f + 1) * full], n, starts, taps, SCALE, MODE[fold]) for f in range(frames)]
        min_amp = float(np.float32(np.median(lin[0])))
        eng = _engine(ksa, n, starts, full, taps, fold, frames, min_amp=min_amp)
        res = {}
        for mode in (ksa.OUT_LINEAR, ksa.OUT_DB, ksa.OUT_DB_CLIP):
            eng.curscan_dev(dev, ksa.FMT_C64, frames, out, out_mode=mode)
            torch.cuda.synchronize()
            res[mode] = out.cpu().numpy()
        eng.close()
        for f in range(frames):
            block, what = x[f * full:(f + 1) * full], "N=%d %s %s frame %d" % (n, fam, fold, f)
            check(res[ksa.OUT_LINEAR][f], lin[f], what=what)
            assert_db(res[ksa.OUT_DB][f], cm.spectrum(block, n, starts, taps, SCALE, MODE[fold], cm.DB, GAIN), what=what + " OUT_DB")
            want = cm.spectrum(block, n, starts, taps, SCALE, MODE[fold], cm.DB_CLIP, GAIN, min_amp)
            assert_db(res[ksa.OUT_DB_CLIP][f], want, what=what + " OUT_DB_CLIP")
            floor = 10 * np.log10(min_amp) - GAIN
            assert np.sum(np.abs(want - floor) < 1e-9) >= n // 4, "the clip level does not bite"


@pytest.mark.parametrize("n", sorted(SIZES))
def test_host_pointer_entries_equal_the_device_entries(ksa, torch_cuda, n):
    """ksa_curscan_c64 / _u8 and ksa_frames_c64 / _u8 on a shuffled geometry (family f; a at 4096) against ksa_curscan_dev /
    ksa_frames_dev on a device copy of the same memory: array_equal (the header: "the same contract ... bit for bit")."""
    torch = torch_cuda
    fam = "f" if "f" in SIZES[n][2] else "a"
    starts, full = geometry(n, SIZES[n][1][0], fam)
    taps, frames = _taps(n), 3
    x = _take(frames * full, off=n % 7).reshape(frames, full)
    raw = _quantized(ksa, x.reshape(-1), ksa.FMT_U8).reshape(frames, 2 * full)
    eng = _engine(ksa, n, starts, full, taps, "AVG", frames)
    out = torch.empty((frames, n), dtype=torch.float32, device="cuda")
    for name, fmt, blocks in (("c64", ksa.FMT_C64, x), ("u8", ksa.FMT_U8, raw)):
        dev = _dev(torch, blocks.reshape(-1))
        eng.curscan_dev(dev, fmt, 1, out)
        torch.cuda.synchronize()
        host = eng.curscan(blocks[0])
        assert np.array_equal(host, out[0].cpu().numpy().astype(np.float64)), "curscan %s" % name
        assert_lin(host, cm.spectrum(_block(blocks[0], name, 0, full), n, starts, taps, SCALE, cm.AVG), what="N=%d curscan %s" % (n, name))
        eng.reset()
        eng.frames_dev(dev, fmt, frames, cur_db=out)
        eng.synchronize()
        dev_db, dev_state = out.cpu().numpy(), eng.state()
        eng.reset()
        host_db, _ = eng.frames(blocks, cur_db=True)
        host_state = eng.state()
        assert np.array_equal(host_db, dev_db), "frames %s" % name
        for c in ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg", "fftHM"):
            assert np.array_equal(host_state[c], dev_state[c]), "frames %s %s" % (name, c)
        want = cm.spectrum(_block(blocks[frames - 1], name, 0, full), n, starts, taps, SCALE, cm.AVG, cm.DB, GAIN)
        assert_db(host_db[frames - 1], want, what="N=%d frames %s" % (n, name))
    eng.close()


@pytest.mark.parametrize("n,fam,frames", [(1024, "a", "pair"), (1024, "f", "pair"), (4096, "a", "grid"), (4096, "e", "grid"), (64, "b", 9), (64, "f", 40)])
def test_frame_stride_zero_repeats_one_block(ksa, torch_cuda, n, fam, frames):
    """check_frames refuses a negative frame_stride only: 0 is the caller's right.  Every frame then reads the same block, so
    every row of a batch larger than the grid must be array_equal to row 0 -- whichever workgroup, pair half or ticket run
    computed it (N = 1024: the pair kernel with its half pair; N = 4096: more frames than resident workgroups; N = 64)."""
    torch = torch_cuda
    grid = _grid(ksa, n)
    frames = {"pair": 2 * grid + 1, "grid": grid + 5}.get(frames, frames)
    starts, full = geometry(n, SIZES[n][1][0], fam)
    taps = _taps(n)
    x = _take(full, off=5)
    out = torch.empty((frames, n), dtype=torch.float32, device="cuda")
    for fold in ("AVG", "RAW"):
        eng = _engine(ksa, n, starts, full, taps, fold, frames)
        for name in ("c64", "s16"):
            src = _quantized(ksa, x, _fmts(ksa)[name])
            out.fill_(-1.0)
            eng.curscan_dev(_dev(torch, src), _fmts(ksa)[name], frames, out, frame_stride=0)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert np.array_equal(got, np.broadcast_to(got[0], got.shape)), "N=%d %s %s: rows differ from row 0" % (n, fold, name)
            assert_lin(got[0], cm.spectrum(_block(src, name, 0, full), n, starts, taps, SCALE, MODE[fold]), what="N=%d %s %s row 0" % (n, fold, name))
        eng.close()


# ---- the polyphase modes --------------------------------------------------------------------------------------------------------
def pfb_starts(shape, n, p):
    k = np.arange(p, dtype=np.int64)
    if shape == "half":          # overlapping segments: an oversampled WOLA bank
        s = k * (n // 2)
    elif shape == "desc":        # descending k*N
        s = (k * n)[::-1].copy()
    elif shape == "plus1":       # off the 16-byte alignment
        s = k * n + 1
    elif shape == "dup":         # a start listed twice
        s = k * n
        s[-1] = s[0]
    elif shape == "except1":     # a ring-size P with starts[k] == k*N except one: must take the generic form
        s = k * n
        s[2] -= 5
    else:
        raise ValueError(shape)
    return s.astype(np.int32)


PFB_SHAPES = {1: ("half", "plus1"), 3: ("half", "desc", "plus1", "dup"), 4: ("half", "desc", "plus1", "dup", "except1"),
              16: ("half", "desc", "plus1", "dup")}
PFB_CASES = [(n, p, shape) for n in (64, 512, 2400) for p in (1, 3, 4, 16) for shape in PFB_SHAPES[p]]
PFB_PATH = {64: 5, 512: 0, 2400: 6}
PFB_FRAMES = 5


def _pfb_run(ksa, torch, eng, n, full, starts, taps, mode, what):
    """Five frames at frame_stride N (the ring form's stride, which these starts must NOT take) and N + 3, all four formats."""
    check = assert_psd if mode == cm.PFB_PSD else assert_lin
    out = torch.empty((PFB_FRAMES, n), dtype=torch.float32, device="cuda")
    for stride in (n, n + 3):
        x = _take((PFB_FRAMES - 1) * stride + full, off=stride % 17)
        for name, fmt in _fmts(ksa).items():
            src = _quantized(ksa, x, fmt)
            out.fill_(-1.0)
            eng.curscan_dev(_dev(torch, src), fmt, PFB_FRAMES, out, frame_stride=stride)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert np.all(got >= 0), "a frame was not written"
            for f in range(PFB_FRAMES):
                want = cm.spectrum(_block(src, name, f * stride, full), n, starts, taps, SCALE, mode)
                check(got[f], want, what="%s %s stride %d frame %d" % (what, name, stride, f))


@pytest.mark.parametrize("case", PFB_CASES, ids=["%d-%d-%s" % c for c in PFB_CASES])
def test_polyphase_fold_on_caller_chosen_starts(ksa, torch_cuda, case):
    """KSA_CUMU_PFB.  choose_plan: pfb_ring_ok needs P in {4, 8, 16} AND starts[k] == k*N for every k; launch_pfb adds
    frame_stride == N.  None of these shapes satisfies it (except1: P = 4 at stride N, one start off by 5), so pfb_fold_kernel --
    the only form that reads the starts -- serves them all, pairing window_starts[k] with tap segment k in list order."""
    n, p, shape = case
    starts = pfb_starts(shape, n, p)
    full = int(starts.max()) + n
    taps = _taps(n, p, seed=p)
    eng = ksa.SpectrumEngine(n, full_size=full, pfb_taps=p, window=taps, starts=starts, mag_scale=SCALE, xres=_xres(n), max_frames=PFB_FRAMES,
                             u8_offset=U8_OFFSET, u8_scale=U8_SCALE)
    assert eng.num_windows == p and np.array_equal(eng._starts32, starts) and eng.mag_scale == SCALE and eng.kernel_info()["path"] == PFB_PATH[n]
    _pfb_run(ksa, torch_cuda, eng, n, full, starts, taps, cm.PFB, "PFB N=%d P=%d %s" % case)
    eng.close()


@pytest.mark.parametrize("case", PFB_CASES, ids=["%d-%d-%s" % c for c in PFB_CASES])
def test_polyphase_spectrometer_takes_k_from_the_largest_start(ksa, torch_cuda, case):
    """KSA_CUMU_PFB_PSD on the same starts with the largest one moved to the middle of the list and a full_size with a ragged
    tail.  pfb_subframes: K = (full_size - max_k(starts) - N) / N + 1 by std::max_element, wherever the maximum is listed; the
    engine's K must be the header's formula, and pfbpsd_fold_kernel reads j*N + starts[k]."""
    n, p, shape = case
    starts = pfb_starts(shape, n, p)
    i, mid = int(np.argmax(starts)), p // 2
    starts[[i, mid]] = starts[[mid, i]]
    assert p < 3 or 0 < int(np.argmax(starts)) < p - 1
    k = 3
    full = int(starts.max()) + k * n + n // 3
    taps = _taps(n, p, seed=p)
    eng = ksa.SpectrumEngine(n, full_size=full, pfb_taps=p, pfb_spectra=1, window=taps, starts=starts, mag_scale=SCALE, xres=_xres(n),
                             max_frames=PFB_FRAMES, u8_offset=U8_OFFSET, u8_scale=U8_SCALE)
    assert eng.pfb_spectra == cm.subframes(full, n, starts) == (full - int(starts.max()) - n) // n + 1 == k
    assert np.array_equal(eng._starts32, starts) and eng.mag_scale == SCALE and eng.kernel_info()["path"] == PFB_PATH[n]
    _pfb_run(ksa, torch_cuda, eng, n, full, starts, taps, cm.PFB_PSD, "PFB_PSD N=%d P=%d %s" % case)
    eng.close()


def test_polyphase_frame_stride_zero(ksa, torch_cuda):
    """frame_stride 0 on the fold kernels (N = 64, P = 4, overlapping segments): every row equals row 0."""
    torch = torch_cuda
    n, p, frames = 64, 4, 37
    starts = pfb_starts("half", n, p)
    full, taps = int(starts.max()) + 2 * n, _taps(n, p)
    x = _take(full, off=3)
    out = torch.empty((frames, n), dtype=torch.float32, device="cuda")
    for spectra, mode, check in ((0, cm.PFB, assert_lin), (1, cm.PFB_PSD, assert_psd)):
        eng = ksa.SpectrumEngine(n, full_size=full, pfb_taps=p, pfb_spectra=spectra, window=taps, starts=starts, mag_scale=SCALE, xres=64, max_frames=frames)
        out.fill_(-1.0)
        eng.curscan_dev(_dev(torch, x), ksa.FMT_C64, frames, out, frame_stride=0)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(got, np.broadcast_to(got[0], got.shape))
        check(got[0], cm.spectrum(x, n, starts, taps, SCALE, mode), what="stride 0 mode %d" % mode)
        eng.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refused_configs_name_their_field_and_leave_a_live_engine_as_it_was(ksa, torch_cuda):
    """validate_config: window starts compared in 64 bits (INT32_MAX + N wraps in int), scan_total_entries in 0 ..
    KSA_MAX_SCAN_TOTAL_ENTRIES (the stitch, row and levels kernels index float[4][total] in int: the bound is derived from that
    indexing, which stays as it is), full_size up to KSA_MAX_FULL_SIZE (32-bit byte offsets of 8-byte samples; one bound for every
    format, since fmt arrives per call), u8_scale finite.  Each refusal: non-zero, null handle, a text of its own naming the field.
    The same fields one step inside are accepted.  An engine that lives through all of it keeps its state and its results."""
    n, frames = 64, 2
    starts, full = geometry(n, 5, "f")
    taps = _taps(n)
    x = _take(frames * full, off=1).reshape(frames, full)
    eng = _engine(ksa, n, starts, full, taps, "AVG", frames)
    eng.frames(x)
    before = eng.state()
    texts = set()
    for name, fields, words in ch.REFUSALS:
        ch.assert_refused(fields, words)
        texts.add(ch.create(**fields)[1])
    assert len(texts) == len(ch.REFUSALS), "two refusals share one text"
    for name, fields in ch.ACCEPTED:
        rc, err, h = ch.create(**fields)
        assert rc == 0 and h.value, "%s: %s" % (name, err)
        ch.destroy(h)
    after = eng.state()
    for c in ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg", "fftHM"):
        assert np.array_equal(before[c], after[c]), c
    assert after["hm_index"] == before["hm_index"] == frames and after["frames"] == frames
    assert_lin(eng.curscan(x[1]), cm.spectrum(x[1], n, starts, taps, SCALE, cm.AVG), what="after the refusals")
    eng.close()
