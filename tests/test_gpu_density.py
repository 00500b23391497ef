"""The density (persistence) histogram on the GPU against its float32 model (tests/density_model.py).  Every comparison is
exact: np.array_equal on int64.  Shapes are the smallest at which the add kernel takes each of its paths: one and several
strips, one and several chunks of rows, strips narrower and wider than a wave, 16-byte and 4-byte loads, g = 1 and g > 1."""
import ctypes as C
import importlib
import re

import numpy as np
import pytest

import density_model as dm
from conftest import load_pkg

pytestmark = pytest.mark.gpu

NBINS = (16, 64, 4096)
LEVELS = (1, 2, 256, 1000)
NROWS = (1, 3, 257, 5000)
RANGE = {1: (-100.0, -50.0), 2: (-100.0, -50.0), 256: (-140.0, 0.0), 1000: (-133.3, 7.1)}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def D():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.density")


def cloud(seed, nrows, nbins, levels, lo, hi):
    """A normal dB cloud around a floor a third of the way up the range, with -inf, +inf, NaN, exact edge values (and their
    float32 neighbours) and values far outside the range injected at random places."""
    rng = np.random.default_rng(seed)
    rows = (lo + (hi - lo) / 3 + (hi - lo) / 12 * rng.standard_normal((nrows, nbins))).astype(np.float32)
    flat = rows.reshape(-1)
    special = np.concatenate([dm.edge_values(levels, lo, hi),
                              np.array([-np.inf, np.inf, np.nan, -1e30, 1e30, -3e38, 3e38, lo - 1e4, hi + 1e4, 0.0, -0.0],
                                       dtype=np.float32)])
    k = max(4, flat.size // 50)
    where = rng.integers(0, flat.size, size=k)
    flat[where] = special[rng.integers(0, len(special), size=k)]
    for j, v in enumerate((np.nan, np.inf, -np.inf, lo, hi)):          # every kind at least once, whatever the draw
        flat[(j * 3) % flat.size] = v
    return rows


def case_list():
    out = []
    for i, nbins in enumerate(NBINS):
        for j, width in enumerate((nbins, nbins // 4, 1)):
            for k, levels in enumerate(LEVELS):
                out.append((nbins, width, levels, NROWS[(i + j + k) % 4]))
    return out


CASES = case_list()


def test_the_cases_cover_every_row_count_with_and_without_shared_columns():
    for nrows in NROWS:
        assert any(c[3] == nrows and c[0] == c[1] for c in CASES) and any(c[3] == nrows and c[0] != c[1] for c in CASES)


# ------------------------------------------------------------------------------------------ 1. against the model
@pytest.mark.parametrize("nbins,width,levels,nrows", CASES)
def test_counts_match_the_model(D, torch_cuda, nbins, width, levels, nrows):
    torch = torch_cuda
    lo, hi = RANGE[levels]
    rows = cloud(nbins * 7 + width * 3 + levels + nrows, nrows, nbins, levels, lo, hi)
    want = dm.histogram(rows, width, levels, lo, hi)
    dens = D.SpectrumDensity(nbins, width, levels, lo, hi)
    dev = torch.from_numpy(rows).cuda()
    dens.add_rows_dev(dev, nrows)
    got, seen = dens.read()
    info = dens.kernel_info()
    dens.close()
    assert got.dtype == np.int64 and got.shape == (levels + 1, width)
    assert seen == nrows
    assert np.array_equal(got.sum(axis=0), np.full(width, nrows * (nbins // width))), "a column lost or gained counts"
    assert np.array_equal(got[levels], want[levels]), "NaN row"
    assert np.array_equal(got, want)
    assert info["threads"] == 256 and info["grid"] >= 1 and info["lds_bytes"] >= (levels + 1) * 4
    assert info["lds_optin"] == (1 if info["lds_bytes"] > 65536 else 0)


@pytest.mark.parametrize("nbins,width,levels", [(48, 48, 5), (48, 12, 7), (18, 18, 3), (18, 9, 3), (18, 1, 2), (2400, 300, 64),
                                                (2400, 2400, 1024)])
def test_sizes_that_are_no_power_of_two(D, torch_cuda, nbins, width, levels):
    """Widths that one strip takes whole, strips whose last one is short, rows whose length is no multiple of four floats
    (the 4-byte form even from an aligned buffer)."""
    torch = torch_cuda
    rows = cloud(nbins + width, 37, nbins, levels, -110.0, -30.0)
    dens = D.SpectrumDensity(nbins, width, levels, -110.0, -30.0)
    dev = torch.from_numpy(rows).cuda()
    dens.add_rows_dev(dev, 37)
    got, seen = dens.read()
    dens.close()
    assert seen == 37 and np.array_equal(got, dm.histogram(rows, width, levels, -110.0, -30.0))


# ------------------------------------------------------------------------------------------ 2. alignment and stride
@pytest.mark.parametrize("nbins,width,levels", [(4096, 4096, 256), (4096, 512, 256), (4096, 4096, 1000), (64, 16, 2), (16, 16, 256), (16, 1, 1)])
def test_unaligned_base_and_odd_stride_count_the_same(D, torch_cuda, nbins, width, levels):
    torch = torch_cuda
    lo, hi = RANGE[levels]
    nrows, stride = 257, nbins + 3
    rows = cloud(nbins + levels, nrows, nbins, levels, lo, hi)
    padded = np.full(1 + nrows * stride, np.nan, dtype=np.float32)       # whatever lies between the rows must not be counted
    padded[1:].reshape(nrows, stride)[:, :nbins] = rows
    dev = torch.from_numpy(padded).cuda()
    a = D.SpectrumDensity(nbins, width, levels, lo, hi)
    a.add_rows_dev(dev[1:], nrows, row_stride=stride)
    assert dev[1:].data_ptr() % 16 == 4
    b = D.SpectrumDensity(nbins, width, levels, lo, hi)
    aligned = torch.from_numpy(rows).cuda()
    b.add_rows_dev(aligned, nrows)
    ca, cb = a.read()[0], b.read()[0]
    a.close(), b.close()
    assert np.array_equal(ca, cb)
    assert np.array_equal(ca, dm.histogram(rows, width, levels, lo, hi))


# ------------------------------------------------------------------------------------------ 3. accumulation
@pytest.mark.parametrize("nbins,width", [(4096, 512), (64, 64)])
def test_calls_accumulate_and_host_rows_equal_device_rows(D, torch_cuda, nbins, width):
    torch = torch_cuda
    levels, (lo, hi) = 256, RANGE[256]
    rows = cloud(99 + nbins, 257, nbins, levels, lo, hi)
    dev = torch.from_numpy(rows).cuda()
    one = D.SpectrumDensity(nbins, width, levels, lo, hi)
    one.add_rows_dev(dev, 257)
    two = D.SpectrumDensity(nbins, width, levels, lo, hi)
    two.add_rows_dev(dev, 100)
    two.add_rows_dev(dev[100:], 157)
    two.add_rows_dev(dev, 0)                                  # a successful no-op
    host = D.SpectrumDensity(nbins, width, levels, lo, hi)
    host.add_rows(rows[:100])
    host.add_rows(rows[100:])
    host.add_rows(rows[:0])
    c1, s1 = one.read()
    c2, s2 = two.read()
    c3, s3 = host.read()
    for d in (one, two, host):
        d.close()
    assert s1 == s2 == s3 == 257
    assert np.array_equal(c1, dm.histogram(rows, width, levels, lo, hi))
    assert np.array_equal(c2, c1) and np.array_equal(c3, c1)


# ------------------------------------------------------------------------------------------ 4. hot cell
@pytest.mark.parametrize("width", [16, 1])
def test_one_cell_takes_more_than_65536_hits(D, torch_cuda, width):
    torch = torch_cuda
    nrows, nbins, levels = 70000, 16, 8
    dev = torch.full((nrows, nbins), -75.0, dtype=torch.float32, device="cuda")
    dens = D.SpectrumDensity(nbins, width, levels, -120.0, -40.0)       # 10 dB per level: -75 is level 4
    dens.add_rows_dev(dev, nrows)
    got, seen = dens.read()
    dens.close()
    want = np.zeros((levels + 1, width), dtype=np.int64)
    want[4, :] = nrows * (nbins // width)
    assert seen == nrows and got[4, 0] > 2 ** 16
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------ 5. decay, merge, reset
def test_decay_merge_reset(D, torch_cuda):
    torch = torch_cuda
    nbins, width, levels, (lo, hi) = 64, 16, 256, RANGE[256]
    rows = cloud(7, 257, nbins, levels, lo, hi)
    base = dm.histogram(rows, width, levels, lo, hi)
    a = D.SpectrumDensity(nbins, width, levels, lo, hi)
    a.add_rows(rows)
    a.decay(3, 4)
    got, seen = a.read()
    assert np.array_equal(got, dm.decay(base, 3, 4)) and seen == 257            # rows_seen is left alone
    assert np.any(got != base)
    a.decay(0, 1)
    assert not a.read()[0].any()
    a.reset()
    a.add_rows(rows)
    # merge: b += a through the zero-copy view of a's counters
    b = D.SpectrumDensity(nbins, width, levels, lo, hi)
    b.add_rows(rows[:100])
    view = torch.as_tensor(a.counts_dev(), device="cuda")
    assert view.dtype == torch.int64 and tuple(view.shape) == (levels + 1, width)
    a.synchronize()
    assert np.array_equal(view.cpu().numpy(), base)
    b.merge_dev(view, rows_seen_add=257)
    got, seen = b.read()
    assert np.array_equal(got, base + dm.histogram(rows[:100], width, levels, lo, hi)) and seen == 357
    # 64-bit path: an object's own read-back merged 34 times doubles it 34 times
    want = base.copy()
    a.reset()
    a.add_rows(rows)
    for _ in range(34):
        back, _ = a.read()
        a.merge_dev(torch.from_numpy(back).cuda())
        want += want
    got, seen = a.read()
    assert want.max() > 2 ** 33 and seen == 257
    assert np.array_equal(got, want)
    big = 2 ** 31 - 1
    a.decay(big, big)
    assert np.array_equal(a.read()[0], want)
    a.decay(1, 3)
    got = a.read()[0]
    assert np.array_equal(got, dm.decay(want, 1, 3))
    assert got.tolist() == [[int(v) // 3 for v in row] for row in want.tolist()]
    a.reset()
    got, seen = a.read()
    assert not got.any() and seen == 0
    a.close(), b.close()


# ------------------------------------------------------------------------------------------ 6. behind the engine
def test_rows_of_the_engine_are_counted_in_stream_order(ksa, D, torch_cuda):
    torch = torch_cuda
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(11)

    def iq(frames, full):
        x = (rng.standard_normal((frames, full)) + 1j * rng.standard_normal((frames, full))).astype(np.complex64) * 0.05
        x += np.exp(2j * np.pi * 0.123 * np.arange(full)).astype(np.complex64)
        return torch.view_as_real(torch.from_numpy(x)).cuda()

    for n, frames, shape, width in ((4096, 64, dict(non_overlap=0.5, window="hanning"), 512),
                                    (64, 64, dict(pfb_taps=4, pfb_spectra=8), 64)):
        eng = ksa.SpectrumEngine(n, max_frames=frames, **shape)
        dev = iq(frames, eng.full_size)
        buf = torch.full((frames, n), float("nan"), dtype=torch.float32, device="cuda")
        dens = D.SpectrumDensity(n, width, 256, -140.0, 0.0)
        torch.cuda.synchronize()
        eng.set_stream(stream.cuda_stream)
        dens.set_stream(stream.cuda_stream)
        eng.frames_dev(dev, ksa.FMT_C64, frames, cur_db=buf)
        dens.add_rows_dev(buf, frames)                       # no synchronisation between the two
        got, seen = dens.read()
        rows = buf.cpu().numpy()
        assert seen == frames and not np.isnan(rows).any()
        assert np.array_equal(got, dm.histogram(rows, width, 256, -140.0, 0.0))
        assert got[1:255].sum() > 0, "the spectrum missed the range: the test would compare clamps only"
        dens.close()
        eng.close()
    # an all-zero block under KSA_OUT_DB is a row of -inf: every count lands in level 0
    n, frames = 64, 3
    eng = ksa.SpectrumEngine(n, non_overlap=0.5, window="hanning", max_frames=frames)
    zeros = torch.zeros((frames, eng.full_size, 2), dtype=torch.float32, device="cuda")
    out = torch.full((frames, n), float("nan"), dtype=torch.float32, device="cuda")
    dens = D.SpectrumDensity(n, 16, 64, -120.0, 0.0)
    torch.cuda.synchronize()
    eng.set_stream(stream.cuda_stream)
    dens.set_stream(stream.cuda_stream)
    eng.curscan_dev(zeros, ksa.FMT_C64, frames, out, out_mode=ksa.OUT_DB)
    dens.add_rows_dev(out, frames)
    got, seen = dens.read()
    assert np.all(np.isneginf(out.cpu().numpy()))
    want = np.zeros((65, 16), dtype=np.int64)
    want[0, :] = frames * 4
    assert np.array_equal(got, want) and seen == frames
    dens.close()
    eng.close()


# ------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_have_their_own_text_and_change_nothing(D, torch_cuda):
    torch = torch_cuda
    lib = D.lib()
    texts = []

    def refused(rc):
        assert rc != 0
        text = lib.ksd_last_error().decode()
        assert text
        texts.append(text)

    nan, inf = float("nan"), float("inf")
    for args in ((0, 8, 8, 16, -1.0, 0.0), (0, 2 ** 20 + 16, 1, 16, -1.0, 0.0), (0, 64, 0, 16, -1.0, 0.0), (0, 64, 48, 16, -1.0, 0.0),
                 (0, 64, 64, 0, -1.0, 0.0), (0, 64, 64, 1025, -1.0, 0.0), (0, 64, 64, 16, nan, 0.0), (0, 64, 64, 16, -1.0, inf),
                 (0, 64, 64, 16, 0.0, 0.0), (0, 64, 64, 16, 1.0, -1.0), (0, 64, 64, 16, 0.0, 1e-45),
                 (0, 2 ** 20, 2 ** 20, 128, -1.0, 0.0)):
        h = C.c_void_p(1)
        refused(lib.ksd_create(*args, C.byref(h)))
        assert h.value is None, args
    # nbins / width / divides / levels / not finite / lo < hi / inv not finite / too many cells: eight rules, eight texts
    assert len({re.sub(r"-?[0-9.e+]+|inf|nan", "#", t) for t in texts}) == 8, texts

    nbins, width, levels, (lo, hi) = 64, 16, 256, RANGE[256]
    rows = cloud(3, 20, nbins, levels, lo, hi)
    dens = D.SpectrumDensity(nbins, width, levels, lo, hi)
    dens.add_rows(rows)
    before, seen_before = dens.read()
    dev = torch.from_numpy(rows).cuda()
    other = torch.ones((levels + 1, width), dtype=torch.int64, device="cuda")
    texts.clear()
    h, p = dens._h, C.c_void_p(dev.data_ptr())
    refused(lib.ksd_add_rows_dev(h, None, nbins, 20))
    refused(lib.ksd_add_rows_dev(h, p, nbins, -1))
    refused(lib.ksd_add_rows_dev(h, p, nbins - 1, 20))
    refused(lib.ksd_add_rows_dev(None, p, nbins, 20))
    refused(lib.ksd_add_rows(h, None, 20))
    refused(lib.ksd_add_rows(h, rows.ctypes.data_as(C.c_void_p), -1))
    for num, den in ((-1, 4), (5, 4), (1, 0), (1, 2 ** 31), (0, -3)):
        refused(lib.ksd_decay(h, num, den))
    refused(lib.ksd_merge_dev(h, None, 0))
    refused(lib.ksd_merge_dev(h, C.c_void_p(other.data_ptr()), -1))
    refused(lib.ksd_read(h, None, None))
    refused(lib.ksd_counts_dev(h, None))
    refused(lib.ksd_reset(None))
    refused(lib.ksd_set_stream(None, None))
    assert len(set(texts)) >= 9, texts
    with pytest.raises(D.KsaError, match="row_stride"):
        dens.add_rows_dev(dev, 20, row_stride=nbins - 1)
    with pytest.raises(D.KsaError):
        dens.add_rows(rows[:, :nbins - 1])
    after, seen_after = dens.read()
    dens.close()
    assert np.array_equal(after, before) and seen_after == seen_before == 20


# ------------------------------------------------------------------------------------------ 8. the command line
def test_cli_density_counts_every_frame_and_leaves_the_state_alone(ksa, D, torch_cuda, tmp_path, capsys):
    K = importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")
    sources = importlib.import_module("prgs-sdr-kspecanal_amd.sources")
    n, frames = 512, 21                                      # 21 = 2 batches of 8 and one of 5
    base = K.handle_args({}, ["zeroSpan", "fftSize", str(n), "iqFormat", "u8"])
    full = base["fullSize"]
    rng = np.random.default_rng(2024)
    t = np.arange(16 * 1024 + frames * full)
    x = 0.4 * np.exp(2j * np.pi * 0.21 * t) + 0.05 * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
    raw = np.empty(2 * t.size, dtype=np.uint8)
    raw[0::2] = np.clip(np.round(x.real * 127.5 + 127.5), 0, 255)
    raw[1::2] = np.clip(np.round(x.imag * 127.5 + 127.5), 0, 255)
    path = tmp_path / "cap_u8.bin"
    raw.tofile(path)
    common = ["zeroSpan", "fftSize", str(n), "iqFormat", "u8", "source", "file:%s" % path, "bPltLevels", "false",
              "bPltHeatMap", "false", "prgLoopCnt", str(frames)]

    # what an engine of the same configuration returns for the same blocks
    src = sources.FileSdr(str(path), iq_format="u8")
    src.read_samples(16 * 1024)                              # the settle samples sdr_setup discards
    blocks = np.array([K.sdr_read(src, full, raw=True) for _ in range(frames)])
    src.close()
    eng = ksa.SpectrumEngine(n, full_size=full, non_overlap=base["curScanNonOverlap"], window=base["theWin"],
                             cumu_mode=base["curScanCumuMode"], gain=base["gain"], min_amp=base["minAmp4Clip"],
                             xres=base["xRes"], max_frames=frames)
    db, _ = eng.frames(blocks, cur_db=True)
    width = eng.hm_width
    eng.close()
    want = dm.histogram(db, width, 64, -120.0, 0.0)
    assert want[1:63].sum() > 0

    def run(extra):
        K.sdr_curscan = K._gpu_curscan
        capsys.readouterr()
        d = K.main(common + extra)
        return d, capsys.readouterr().out

    for batch in ("8", "1"):
        plain, _ = run(["frameBatch", batch])
        save = tmp_path / ("f%s.npy" % batch)
        d, out = run(["frameBatch", batch, "density", "64:-120:0", "densitySave", str(save)])
        saved = np.load(save)
        assert saved.dtype == np.int64 and np.array_equal(saved, want), batch
        assert np.array_equal(d["density"], want[:64]) and np.array_equal(d["densityNaN"], want[64])
        assert d["densityRows"] == frames and np.array_equal(d["densityEdges"], D.level_edges(64, -120.0, 0.0))
        assert re.search(r"^INFO:zero_span: density rows \[%d\]" % frames, out, flags=re.M)
        for k in ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg", "fftHM"):
            assert np.array_equal(d[k], plain[k]), (batch, k)              # bit for bit
        assert d["fftHMIndex"] == plain["fftHMIndex"] == frames % 128
