"""GPU tests of the kernels' precision, bin by bin, on every kernel path: the catalogues of test_gpu_psd.py and test_gpu_pfb.py
under white noise, single impulses and a kaiser-windowed tone, and the dB stage of ksa_frames_dev.

One rule for every comparison (precision_model.py):   metric(device) <= MARGIN * metric(fp32 model on the CPU),
both taken against the float64 reference on the same input.  No bound is a fixed number and nothing here reads a file of
ratios: the model runs beside every case.  `assert_lin` at 1e-5 of the strongest bin stays the project's published tolerance
(test_gpu_parity.py and the every-path tests); this file is the regression guard under it.

Where this file chooses for itself:
  * impulse frames do not overlap (frame stride = fullSize; the polyphase stream: one impulse per P segments), so that every
    frame holds exactly one nonzero sample whatever the catalogue's stride is; the frame COUNT follows the catalogue's rules;
  * the impulse positions count from the start of the LAST window of the block.  AVG weighs window k of W by 2^-(W-k), and the
    first of 650 windows is below anything float32 holds; and an impulse at a small offset into the first window meets only
    the left end of every window that holds it, which under kaiser(64) is below fp32's range (precision_model.FP32_SAFE), where
    the earlier windows of an overlapped block see one near the last window's start at their centres;
  * the polyphase "chunk" case runs three frames here (the largest buffer is N = 2^20 with a few frames); the chunk boundary is
    test_gpu_pfb.py's and test_gpu_pfbpsd.py's subject, it is bookkeeping and no arithmetic.

KSA_PRECISION_REPORT=<file> writes the table of ratios that test_report_the_ratios prints."""
import functools
import os

import numpy as np
import pytest

import ksa_oracle as orc
import pfb_helper as pfb
import precision_model as pm
from test_gpu_parity import GAIN
from test_gpu_pfb import PATHS as PFB_PATHS
from test_gpu_psd import PATHS as ENGINE_PATHS

pytestmark = pytest.mark.gpu

MAX_BYTES = 256 << 20
REPORT = []                                   # (case, path, input, metric, device, model, ratio)
FAMILIES = ("white", "impulse", "floor")
DB_CASES = [c for c in ENGINE_PATHS if (c[0], c[2], c[3], c[4]) in {
    (64, 0.5, "hanning", 4), (1000, 0.5, "hanning", 3), (1024, 0.5, "hanning", "pair"), (4096, 0.5, "hanning", "fill"),
    (16384, 0.25, "hanning", "fill"), (65536, 0.25, "hanning", 1)}]
# the numeric floor: the kaiser cases of the engine catalogue and one kaiser case at each size it has none for
FLOOR_CASES = [c for c in ENGINE_PATHS if c[3] == "kaiser"] + [
    (4096, 8192, 0.5, "kaiser", "fill", 0, "packed butterflies (50 % overlap, unsplit)"),
    (8192, 16384, 0.5, "kaiser", 2, 3, "32 points per thread"),
    (65536, 131072, 0.5, "kaiser", 1, 2, "radix-16 first stage, 4096-point second stage"),
    (1048576, 2097152, 1.0, "kaiser", 1, 2, "radix-64 first stage"),
]


def _eid(c):
    return "%d-%s-%s-%s" % (c[0], c[2], c[3], c[4])


def _pid(c):
    return "pfb-%d-%d-%s" % (c[0], c[1], c[3])


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _xres(n):
    return n if n & (n - 1) else min(n, 512)


def _dev(torch, x):
    x = np.ascontiguousarray(x)
    if x.dtype == np.complex64:
        return torch.view_as_real(torch.from_numpy(x.reshape(-1))).to("cuda")
    return torch.from_numpy(x.reshape(-1)).to("cuda")


@functools.lru_cache(maxsize=4)
def _white(total, seed):
    return pm.white(total, seed)


@functools.lru_cache(maxsize=4)
def _tone(total):
    return pm.tone(total)


def _spread(frames, most=6):
    return sorted(set(np.linspace(0, frames - 1, min(frames, most)).astype(int)))


def _probe(ksa, path, **kw):
    """kernel_info of the configuration, with the path asserted as the catalogue states it."""
    probe = ksa.SpectrumEngine(**kw)
    info = probe.kernel_info()
    probe.close()
    assert info["path"] == path, info
    return info


def _engine_frames(case, info):
    """(frames, stride) by the rules of test_gpu_psd.py."""
    frames, stride = case[4], case[1]
    if frames == "pair":
        frames, stride = 2 * info["grid"] + 1, 64
    elif frames == "fill":
        frames, stride = info["grid"] // 2 + 3, 512
    return frames, stride


def _pfb_frames(case, info):
    frames = case[3]
    if frames == "pair":
        return 2 * info["grid"] + 1
    if frames == "fill":
        return info["grid"] // 2 + 3
    if frames == "chunk":
        return 3
    return frames


class Tally:
    """The comparisons of one test: every one goes to the report, the failures are raised together at the end."""

    def __init__(self, case, path, family):
        self.case, self.path, self.family, self.bad = case, path, family, []

    def add(self, metric, device, model):
        ok, ratio = pm.within(device, model, self.path)
        REPORT.append((self.case, self.path, self.family, metric, device, model, ratio))
        print("%-28s path %d %-8s %-14s device %.3e model %.3e ratio %.2f" % (self.case, self.path, self.family, metric, device, model, ratio))
        if not ok:
            self.bad.append("%s: device %.3e > %g x model %.3e (ratio %.2f)" % (metric, device, pm.margin(self.path), model, ratio))

    def close(self):
        assert not self.bad, "%s path %d %s: %s" % (self.case, self.path, self.family, "; ".join(self.bad))


def _run(torch, eng, ksa, dev, fmt, frames, n, stride):
    out = torch.full((frames, n), -1.0, dtype=torch.float32, device="cuda")
    eng.curscan_dev(dev, fmt, frames, out, frame_stride=stride)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got >= 0), "a frame was not written"
    return got


def _lin(mode, v):
    """PSD results are compared as amplitudes, as assert_psd does."""
    return np.sqrt(np.asarray(v, dtype=np.float64)) if mode == "PSD" else np.asarray(v, dtype=np.float64)


def _compare_frames(tally, tag, got, blocks, n, win, mode, q, metrics):
    """Worst figure over the frames in `blocks` (frame index -> samples), device and model each against the reference."""
    worst = {m: [0.0, 0.0] for m in metrics}
    for f, block in blocks.items():
        want = _lin(mode, pm.reference(block, n, win, mode, q))
        model = _lin(mode, pm.yardstick(block, n, win, mode, q))
        for m in metrics:
            fn = getattr(pm, m)
            worst[m][0] = max(worst[m][0], fn(_lin(mode, got[f]), want))
            worst[m][1] = max(worst[m][1], fn(model, want))
    for m in metrics:
        tally.add("%s %s" % (tag, m), *worst[m])


# ------------------------------------------------------------------------------------------------ a. white input
@pytest.mark.parametrize("case", ENGINE_PATHS, ids=[_eid(c) for c in ENGINE_PATHS])
def test_white_input_engine(ksa, torch_cuda, case):
    """AVG and PSD of every engine case on tone-free noise, complex64; uint8 as well at N = 64, where its kernel differs."""
    torch = torch_cuda
    n, full, q, window, _, path, _ = case
    win = orc.window_table(window, n)
    tally = Tally(_eid(case), path, "white")
    for mode in ("AVG", "PSD"):
        kw = dict(fft_size=n, full_size=full, non_overlap=q, window=window, cumu_mode=mode, xres=_xres(n))
        frames, stride = _engine_frames(case, _probe(ksa, path, **kw))
        x = _white((frames - 1) * stride + full, 100 + n)
        eng = ksa.SpectrumEngine(max_frames=frames, **kw)
        got = _run(torch, eng, ksa, _dev(torch, x), ksa.FMT_C64, frames, n, stride)
        _compare_frames(tally, mode, got, {f: x[f * stride:f * stride + full] for f in _spread(frames)}, n, win, mode, q,
                        ("rms_err", "max_err"))
        if n == 64:
            raw = orc.quantize_u8(x)
            got = _run(torch, eng, ksa, _dev(torch, raw), ksa.FMT_U8, frames, n, stride)
            x8 = orc.unpack_u8(raw)
            _compare_frames(tally, mode + " u8", got, {f: x8[f * stride:f * stride + full] for f in _spread(frames)}, n, win, mode, q,
                            ("rms_err", "max_err"))
        eng.close()
    tally.close()


@pytest.mark.parametrize("case", PFB_PATHS, ids=[_pid(c) for c in PFB_PATHS])
def test_white_input_pfb(ksa, torch_cuda, case):
    """Frames at stride N over one noise stream; uint8 as well at N = 64 and at N = 512 (P = 4: the generic fold for uint8)."""
    torch = torch_cuda
    n, p, window, _, path, _ = case
    kw = dict(fft_size=n, pfb_taps=p, window=window, xres=_xres(n))
    frames = _pfb_frames(case, _probe(ksa, path, **kw))
    taps = pfb.prototype(n, p, window)
    x = _white((frames - 1 + p) * n, 200 + n)
    tally = Tally(_pid(case), path, "white")
    eng = ksa.SpectrumEngine(max_frames=frames, **kw)
    got = _run(torch, eng, ksa, _dev(torch, x), ksa.FMT_C64, frames, n, n)
    _compare_frames(tally, "PFB", got, {f: x[f * n:(f + p) * n] for f in _spread(frames)}, n, taps, "PFB", None, ("rms_err", "max_err"))
    if n in (64, 512):
        raw = orc.quantize_u8(x)
        got = _run(torch, eng, ksa, _dev(torch, raw), ksa.FMT_U8, frames, n, n)
        x8 = orc.unpack_u8(raw)
        _compare_frames(tally, "PFB u8", got, {f: x8[f * n:(f + p) * n] for f in _spread(frames)}, n, taps, "PFB", None,
                        ("rms_err", "max_err"))
    eng.close()
    tally.close()


# ------------------------------------------------------------------------------------------------ b. impulses
def _impulse_tally(tally, tag, got, want_rows, model_rows, scale):
    """got: [frames][n] of the device, frame f against row f % L; the model's rows against the same truth."""
    L = len(want_rows)
    want = np.asarray(want_rows)[np.arange(len(got)) % L]
    device, held = pm.impulse_err(got, want, scale)
    model, _ = pm.impulse_err(np.asarray(model_rows), np.asarray(want_rows), scale)
    # (without overlap, kaiser(64) leaves 16 of the 39 positions of N = 1024 in range: its taps, not the kernels)
    assert 4 * held >= len(got), "%s: only %d of %d frames lie in fp32's range" % (tag, held, len(got))
    tally.add("%s bin_err" % tag, device, model)


@pytest.mark.parametrize("case", ENGINE_PATHS, ids=[_eid(c) for c in ENGINE_PATHS])
def test_impulses_engine(ksa, torch_cuda, case):
    """One impulse per frame, every bin relative to itself, AVG and MAX.  Frame f holds position f % L of the list."""
    torch = torch_cuda
    n, full, q, window, _, path, _ = case
    win = orc.window_table(window, n)
    pos = pm.impulse_positions(n)
    tally = Tally(_eid(case), path, "impulse")
    for mode in ("AVG", "MAX"):
        kw = dict(fft_size=n, full_size=full, non_overlap=q, window=window, cumu_mode=mode, xres=_xres(n))
        frames = max(len(pos), _engine_frames(case, _probe(ksa, path, **kw))[0])
        assert frames * full * 8 <= MAX_BYTES
        starts, scale = pm.geometry(mode, n, full, q, win)
        base = int(starts[-1])
        x = pm.impulses(frames, full, [base + v for v in pos])
        eng = ksa.SpectrumEngine(max_frames=frames, **kw)
        got = _run(torch, eng, ksa, _dev(torch, x), ksa.FMT_C64, frames, n, full)
        eng.close()
        want = [pm.reference(x[i], n, win, mode, q) for i in range(len(pos))]
        model = [pm.yardstick(x[i], n, win, mode, q) for i in range(len(pos))]
        _impulse_tally(tally, mode, got, want, model, scale)
    tally.close()


@pytest.mark.parametrize("case", PFB_PATHS, ids=[_pid(c) for c in PFB_PATHS])
def test_impulses_pfb(ksa, torch_cuda, case):
    """A stream at stride N with one impulse in every P-th segment: every frame folds exactly one nonzero sample, at each tap
    segment in turn.  Frame f sees block ceil(f / P) at tap segment (-f) % P."""
    torch = torch_cuda
    n, p, window, _, path, _ = case
    kw = dict(fft_size=n, pfb_taps=p, window=window, xres=_xres(n))
    need = _pfb_frames(case, _probe(ksa, path, **kw))
    taps = pfb.prototype(n, p, window)
    pos = pm.impulse_positions(n)
    L = len(pos)
    blocks = max(L, -(-(need - 1) // p)) + 1
    frames = (blocks - 1) * p + 1
    assert blocks * p * n * 8 <= MAX_BYTES
    x = pm.impulses(blocks, p * n, pos).reshape(-1)
    eng = ksa.SpectrumEngine(max_frames=frames, **kw)
    got = _run(torch, eng, ksa, _dev(torch, x), ksa.FMT_C64, frames, n, n)
    eng.close()
    # frames 1 .. L * P hold every (position, tap segment) pair once; later frames repeat them with period L * P
    want = [pm.reference(x[f * n:(f + p) * n], n, taps, "PFB") for f in range(1, L * p + 1)]
    model = [pm.yardstick(x[f * n:(f + p) * n], n, taps, "PFB") for f in range(1, L * p + 1)]
    tally = Tally(_pid(case), path, "impulse")
    _impulse_tally(tally, "PFB", got[1:], want, model, pfb.scale(taps))
    tally.close()


# ------------------------------------------------------------------------------------------------ c. the numeric floor
@pytest.mark.parametrize("case", FLOOR_CASES, ids=[_eid(c) for c in FLOOR_CASES])
def test_numeric_floor_under_the_kaiser_window(ksa, torch_cuda, case):
    """A noise-free tone under kaiser(beta = 64): the truth away from the main lobe is at -174 dBc (the complex64 rounding of
    the samples), so what the device shows there is its own arithmetic: the instrument's spur-free range."""
    torch = torch_cuda
    n, full, q, window, _, path, _ = case
    win = orc.window_table(window, n)
    kw = dict(fft_size=n, full_size=full, non_overlap=q, window=window, cumu_mode="AVG", xres=_xres(n))
    frames, stride = _engine_frames(case, _probe(ksa, path, **kw))
    x = _tone((frames - 1) * stride + full)
    eng = ksa.SpectrumEngine(max_frames=frames, **kw)
    got = _run(torch, eng, ksa, _dev(torch, x), ksa.FMT_C64, frames, n, stride)
    eng.close()
    tally = Tally(_eid(case), path, "floor")
    fe, sp = [0.0, 0.0], [0.0, 0.0]
    for f in _spread(frames):
        block = x[f * stride:f * stride + full]
        want, model = pm.reference(block, n, win, "AVG", q), pm.yardstick(block, n, win, "AVG", q)
        fe = [max(fe[0], pm.floor_err(got[f], want)), max(fe[1], pm.floor_err(model, want))]
        sp = [max(sp[0], pm.spur(got[f], want, n)), max(sp[1], pm.spur(model, want, n))]
    tally.add("floor_err", *fe)
    tally.add("spur", *sp)
    print("N = %d: spur-free range %.1f dBc on the device, %.1f dBc in the fp32 model" % (n, 20 * np.log10(sp[0]), 20 * np.log10(sp[1])))
    tally.close()


# ------------------------------------------------------------------------------------------------ d. the dB stage
@pytest.mark.parametrize("case", DB_CASES, ids=[_eid(c) for c in DB_CASES])
def test_db_stage_on_typical_bins(ksa, torch_cuda, case):
    """ksa_frames_dev's per-frame dB rows on white input, on the bins at or above 0.1 * rms of the reference."""
    torch = torch_cuda
    n, full, q, window, _, path, _ = case
    win = orc.window_table(window, n)
    kw = dict(fft_size=n, full_size=full, non_overlap=q, window=window, cumu_mode="AVG", gain=GAIN, xres=_xres(n))
    frames, stride = _engine_frames(case, _probe(ksa, path, **kw))
    x = _white((frames - 1) * stride + full, 100 + n)
    eng = ksa.SpectrumEngine(max_frames=frames, **kw)
    rows = torch.full((frames, n), 7.0, dtype=torch.float32, device="cuda")
    eng.frames_dev(_dev(torch, x), ksa.FMT_C64, frames, cur_db=rows, frame_stride=stride)
    eng.synchronize()
    eng.close()
    rows = rows.cpu().numpy()
    tally = Tally(_eid(case), path, "db")
    worst = [0.0, 0.0]
    for f in _spread(frames):
        block = x[f * stride:f * stride + full]
        want = pm.reference(block, n, win, "AVG", q)
        want_db, model_db = pm.to_db(want, GAIN), pm.to_db(pm.yardstick(block, n, win, "AVG", q), GAIN)
        assert np.array_equal(np.isnan(rows[f]), np.isnan(want_db)) and np.array_equal(np.isneginf(rows[f]), np.isneginf(want_db))
        assert np.array_equal(np.isposinf(rows[f]), np.isposinf(want_db))
        mask = pm.typical_bins(want)
        assert np.mean(mask) >= pm.SHARE, np.mean(mask)
        worst = [max(worst[0], pm.db_err(rows[f], want_db, mask)), max(worst[1], pm.db_err(model_db, want_db, mask))]
    tally.add("db_err", *worst)
    tally.close()


# ------------------------------------------------------------------------------------------------ the record
def test_report_the_ratios():
    """Prints the table and the largest ratio per path, writes it where KSA_PRECISION_REPORT says, and asserts that every path
    the two catalogues name was seen under every input family."""
    lines = ["%-28s %4s %-8s %-16s %11s %11s %7s" % ("case", "path", "input", "metric", "device", "model", "ratio")]
    lines += ["%-28s %4d %-8s %-16s %11.3e %11.3e %7.2f" % r for r in REPORT]
    lines.append("")
    for path in sorted({r[1] for r in REPORT}):
        rows = [r for r in REPORT if r[1] == path]
        top = max(rows, key=lambda r: r[6])
        lines.append("path %d: largest ratio %.2f (%s, %s, %s) over %d comparisons, margin %g" % (
            path, top[6], top[0], top[2], top[3], len(rows), pm.margin(path)))
    for r in REPORT:
        if r[3] == "spur":
            lines.append("floor %-28s path %d: %.1f dBc on the device, %.1f dBc in the fp32 model" % (
                r[0], r[1], 20 * np.log10(r[4]), 20 * np.log10(r[5])))
    text = "\n".join(lines) + "\n"
    print(text)
    if os.environ.get("KSA_PRECISION_REPORT"):
        with open(os.environ["KSA_PRECISION_REPORT"], "w") as fh:
            fh.write(text)
    named = {c[5] for c in ENGINE_PATHS} | {c[4] for c in PFB_PATHS}
    for family in FAMILIES:
        seen = {r[1] for r in REPORT if r[2] == family}
        assert named <= seen, "%s input never ran on path(s) %s" % (family, sorted(named - seen))
    assert {r[0] for r in REPORT if r[2] == "db"} == {_eid(c) for c in DB_CASES} and len(DB_CASES) == 6
