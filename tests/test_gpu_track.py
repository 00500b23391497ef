"""The emission tracker on the GPU against its model (tests/track_model.py).  Every comparison is exact: the records byte for
byte (which is np.array_equal on every integer field and the bits of peak_db and floor_db), both totals and every label.  The
shapes are the smallest at which the kernels can go wrong: none and one span, one row, list lengths on either side of one
workgroup (256) and of four, a length that takes several workgroups of the scan's per-thread chunks (65 537), the deepest parent
chain, the widest fan-in onto one root, merges that arrive last, and rows beyond 2^33."""
import functools
import importlib

import numpy as np
import pytest

import detect_model as dm
import track_model as tm
from conftest import load_pkg

pytestmark = pytest.mark.gpu

NBINS = 64
RANDOM_N = (255, 256, 257, 1023, 1024, 1025, 65537)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def X():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.track")


@functools.lru_cache(maxsize=None)
def random_list():
    """The seeded random occupancy, rows x 64 bins at p = 0.18: 66 000 spans or so, of which the tests link prefixes."""
    s = tm.random_occupancy(7400, NBINS, 0.18, seed=20260)
    assert len(s) >= max(RANDOM_N)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def model(n, row_gap=1, bin_slop=1, min_rows=1, min_spans=1, capacity=1 << 20):
    """The model on the first n spans of the random list, computed once per parameter set and shared."""
    s = random_list()[:n]
    return tm.link(s, NBINS, int(s["row"][-1]) + 1, row_gap, bin_slop, min_rows, min_spans, capacity)


def run(X, spans, nbins, row_end, stream=None, **kw):
    """One host-form link on a fresh object: (records, tracks_total, components_total, labels)."""
    trk = X.EmissionTracker(nbins, max_spans=max(len(spans), 1), stream=stream, **kw)
    try:
        labels = trk.link(spans, row_end)
        rec, total, comps = trk.tracks()
        assert np.array_equal(labels, trk.labels())
        return rec, total, comps, labels
    finally:
        trk.close()


def agree(got, want):
    rec, total, comps, labels = got
    assert (total, comps) == (want[1], want[2]), ((total, comps), want[1:3])
    assert np.array_equal(labels, want[3])
    assert rec.dtype == tm.TRACK_DTYPE and len(rec) == len(want[0])
    for name in tm.TRACK_DTYPE.names:
        a, b = rec[name], want[0][name]
        if a.dtype.kind == "f":
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), name
    assert tm.same_records(rec, want[0])


def check(X, rows_or_spans, nbins=NBINS, row_end=None, **kw):
    s = rows_or_spans if isinstance(rows_or_spans, np.ndarray) else tm.spans_of(rows_or_spans)
    end = (int(s["row"].max()) + 1 if len(s) else 0) if row_end is None else row_end
    want = tm.link(s, nbins, end, **{"capacity": 4096, **kw})
    assert want[4] == 0
    agree(run(X, s, nbins, end, **kw), want)
    return want


def to_device(torch, spans):
    return torch.from_numpy(np.ascontiguousarray(spans).view(np.uint8).copy()).to("cuda:0")


# ------------------------------------------------------------------------------------------ the smallest lists
def test_no_span_one_span_and_one_row(X, torch_cuda):
    want = check(X, [])
    assert want[1:3] == (0, 0)
    want = check(X, [(7, 3, 9, -41.5, -77.25, 5)], row_end=9)
    assert want[1:3] == (1, 1) and want[0]["flags"][0] == 0 and want[0]["cells"][0] == 7
    want = check(X, [(7, 3, 9, -41.5, -77.25, 5)], row_end=8)
    assert want[0]["flags"][0] == tm.FLAG_OPEN_END
    want = check(X, [(2, 4 * k, 4 * k + 2) for k in range(16)], bin_slop=8)          # one row: never adjacent
    assert want[1:3] == (16, 16)
    trk = X.EmissionTracker(NBINS)
    info = trk.kernel_info()
    assert info["threads"] == 256 and info["launches"] == 8 and info["grid"] == (1 << 20) // 256 and info["vgprs"] > 0
    trk.close()


def test_a_chain_of_5000_rows_is_one_track(X, torch_cuda):
    rng = np.random.default_rng(3)
    s = tm.spans_of([(r, 20 + (r % 3), 24 + (r % 5)) for r in range(5000)])
    s["peak_db"] = (np.round(rng.normal(-50, 3, len(s)) * 2) / 2).astype(np.float32)
    want = check(X, s)
    assert want[1:3] == (1, 1) and want[0]["nspans"][0] == 5000 and want[0]["row_last"][0] == 4999 and set(want[3]) == {0}


def test_fan_in_of_8192_spans_onto_one_root(X, torch_cuda):
    rows = [(0, 2 * k, 2 * k) for k in range(8192)] + [(1, 0, 16383)]
    want = check(X, rows, nbins=16384)
    assert want[1:3] == (1, 1) and want[0]["nspans"][0] == 8193 and want[0]["first_span"][0] == 0
    rows = [(0, 0, 16383)] + [(1, 2 * k, 2 * k) for k in range(8192)]              # and fan-out: one thread walks them all
    assert check(X, rows, nbins=16384)[1:3] == (1, 1)


def test_a_comb_whose_teeth_join_in_its_last_row_gets_the_lowest_label(X, torch_cuda):
    teeth, rows_n = 300, 40
    rows = [(r, 4 * t, 4 * t + 1) for r in range(rows_n) for t in range(teeth)] + [(rows_n, 0, 4 * teeth - 1)]
    want = check(X, rows, nbins=4 * teeth)
    assert want[1:3] == (1, 1) and want[0]["first_span"][0] == 0 and want[0]["nspans"][0] == teeth * rows_n + 1
    assert check(X, rows[:-1], nbins=4 * teeth)[1:3] == (teeth, teeth)


@pytest.mark.parametrize("slop,tracks", [(0, 600), (1, 1)])
def test_a_staircase_needs_bin_slop_1(X, torch_cuda, slop, tracks):
    rows = [(r, 2 * r, 2 * r + 1) for r in range(600)]                             # every step abuts the one before
    want = check(X, rows, nbins=2048, bin_slop=slop)
    assert want[1:3] == (tracks, tracks)


# ------------------------------------------------------------------------------------------ the random mix
@pytest.mark.parametrize("n", RANDOM_N)
def test_random_occupancy(X, torch_cuda, n):
    s = random_list()[:n]
    want = model(n)
    assert want[4] == 0 and want[0]["nspans"].max() >= 12 and np.count_nonzero(want[0]["nspans"] == 1) >= 5
    agree(run(X, s, NBINS, int(s["row"][-1]) + 1, row_gap=1, bin_slop=1, capacity=1 << 20), want)


def test_capacity_smaller_than_tracks_total_and_the_filters(X, torch_cuda):
    n = 1025
    s = random_list()[:n]
    end = int(s["row"][-1]) + 1
    want = model(n, capacity=7)
    assert want[1] > 7 and len(want[0]) == 7 and want[3].max() == want[1] - 1
    agree(run(X, s, NBINS, end, row_gap=1, bin_slop=1, capacity=7), want)
    for kw in (dict(min_rows=3), dict(min_spans=4), dict(min_rows=2, min_spans=6)):
        want = model(n, **kw)
        assert 0 < want[1] < want[2] and (want[3] == -1).any()
        agree(run(X, s, NBINS, end, row_gap=1, bin_slop=1, capacity=1 << 20, **kw), want)


def test_rows_beyond_2_to_the_33(X, torch_cuda):
    s = tm.random_occupancy(60, NBINS, 0.18, seed=8, row0=2 ** 33 + 5)
    s["row"][len(s) // 2:] += 2 ** 31                                               # and a jump no int32 difference holds
    want = check(X, s, row_gap=1, bin_slop=1)
    assert want[0]["row_first"].min() > 2 ** 33 and want[0]["row_last"].max() > 2 ** 33 + 2 ** 31
    far = tm.spans_of([(5, 1, 2), (5 + 2 ** 32, 1, 2), (6 + 2 ** 32, 1, 2)])      # a difference of 2^32 is no difference of 0
    assert check(X, far, row_gap=1024)[1:3] == (2, 2)


def test_a_second_link_replaces_the_first_and_params_and_clear(X, torch_cuda):
    s = random_list()[:1500]
    trk = X.EmissionTracker(NBINS, row_gap=1, bin_slop=1, capacity=1 << 12, max_spans=2048)
    try:
        for n in (1500, 300, 1024, 1024):                                          # shorter, longer, and once more: idempotent
            labels = trk.link(s[:n], int(s["row"][n - 1]) + 1)
            agree(trk.tracks() + (labels,), tm.link(s[:n], NBINS, int(s["row"][n - 1]) + 1, 1, 1, capacity=1 << 12))
        trk.set_params(row_gap=0, bin_slop=0, min_spans=2)
        labels = trk.link(s[:700], int(s["row"][699]) + 1)
        agree(trk.tracks() + (labels,), tm.link(s[:700], NBINS, int(s["row"][699]) + 1, 0, 0, 1, 2, capacity=1 << 12))
        with pytest.raises(X.KsaError, match="row_gap 2000 outside"):
            trk.set_params(row_gap=2000)
        assert trk.params == (0, 0, 1, 2)
        with pytest.raises(X.KsaError, match="exceeds max_spans 2048"):
            trk.link(random_list()[:2049], 10 ** 6)
        with pytest.raises(X.KsaError, match="row_end -1 must be >= 0"):
            trk.link(s[:5], -1)
        assert trk.counts()["tracks_total"] > 0                                    # refusals leave the result alone
        trk.clear()
        assert trk.counts() == dict(stored=0, tracks_total=0, components_total=0, bad_spans=0) and len(trk.labels()) == 0
    finally:
        trk.close()


# ------------------------------------------------------------------------------------------ the device form
def test_n_dev_smaller_and_larger_than_n_max_and_a_second_stream(X, torch_cuda):
    torch = torch_cuda
    n_max = 1025
    s = random_list()[:n_max]
    dev = to_device(torch, s)
    labels = torch.full((n_max,), 7, dtype=torch.int32, device="cuda:0")
    side = torch.cuda.Stream(device="cuda:0")
    for stream in (None, side.cuda_stream):
        trk = X.EmissionTracker(NBINS, row_gap=1, bin_slop=1, capacity=1 << 12, max_spans=n_max, stream=stream)
        try:
            for n_dev, n in ((600, 600), (n_max, n_max), (10 ** 12, n_max), (0, 0), (-3, 0), (None, n_max), (257, 257)):
                cnt = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int64, device="cuda:0")
                torch.cuda.synchronize()
                end = int(s["row"][n - 1]) + 1 if n else 0
                trk.link_dev(dev, n_max, cnt, end, labels=labels)
                trk.synchronize()
                got = trk.tracks() + (labels.cpu().numpy()[:n],)
                agree(got, tm.link(s[:n], NBINS, end, 1, 1, capacity=1 << 12) if n not in RANDOM_N else model(n, capacity=1 << 12))
                assert np.all(labels.cpu().numpy()[n:] == -1) and np.array_equal(trk.labels(), got[3])
            with pytest.raises(X.KsaError, match="n_max 1026 exceeds max_spans 1025"):
                trk.link_dev(dev, n_max + 1, None, 10)
            # the record buffer and the counters where they lie
            rec_dev = torch.as_tensor(trk.tracks_view(), device="cuda:0").cpu().numpy()
            cnt_dev = torch.as_tensor(trk.counters_view(), device="cuda:0").cpu().numpy()
            want = model(257, capacity=1 << 12)
            assert list(cnt_dev) == [want[1], want[2], 0, 257]
            assert rec_dev[:want[1]].tobytes() == want[0].tobytes()
        finally:
            trk.close()


def test_an_unsorted_list_and_an_overlapping_pair_link_nothing(X, torch_cuda):
    torch = torch_cuda
    s = random_list()[:1025].copy()
    unsorted = s.copy()
    unsorted[[400, 700]] = unsorted[[700, 400]]
    overlap = s.copy()
    k = int(np.flatnonzero(overlap["row"][1:] == overlap["row"][:-1])[0]) + 1      # the second span of some row
    overlap["bin_lo"][k] = overlap["bin_hi"][k - 1]
    beyond = s.copy()
    beyond["bin_hi"][1000] = NBINS
    end = int(s["row"][-1]) + 1
    for broken, row_end in ((unsorted, end), (overlap, end), (beyond, end), (s, end - 1)):
        bad = tm.bad_indices(broken, NBINS, row_end)
        want = tm.link(broken, NBINS, row_end, 1, 1)
        assert len(bad) == want[4] > 0
        trk = X.EmissionTracker(NBINS, row_gap=1, bin_slop=1, max_spans=2048)
        try:
            good = trk.link(s, end)                     # a good result first: the bad link replaces it
            agree(trk.tracks() + (good,), model(1025, capacity=4096))
            with pytest.raises(X.KsaError, match=r"span %d \(row" % bad[0]):       # the host form names the first offender
                trk.link(broken, row_end)
            assert trk.counts()["tracks_total"] == model(1025)[1]                  # and leaves the state alone
            labels = torch.full((len(broken),), 7, dtype=torch.int32, device="cuda:0")
            dev = to_device(torch, broken)
            torch.cuda.synchronize()
            trk.link_dev(dev, len(broken), None, row_end, labels=labels)
            assert trk.counts() == dict(stored=0, tracks_total=0, components_total=0, bad_spans=len(bad))
            assert np.all(labels.cpu().numpy() == -1) and np.all(trk.labels() == -1) and len(trk.labels()) == len(broken)
            with pytest.raises(X.KsaError, match="%d spans of the linked list" % len(bad)):
                trk.tracks()
        finally:
            trk.close()


# ------------------------------------------------------------------------------------------ end to end behind the detector
def scene():
    """[64][1024] dB: a dithered flat floor at -90 dB, a carrier in bins 299..301 of every row, a burst in bins 600..607 of rows
    20..29, a chirp that moves one bin a row from bin 702 in row 2 to bin 761 in row 61, and a hopper that dwells 4 rows on each
    of 16 channels 12 bins apart."""
    rng = np.random.default_rng(11)
    db = (-90.0 + rng.uniform(-0.5, 0.5, (64, 1024))).astype(np.float32)
    db[:, 299:302] = -60.0
    db[:, 300] = -58.0
    db[20:30, 600:608] = -62.0
    for r in range(2, 62):
        db[r, 700 + r] = -61.0
    for r in range(64):
        at = 40 + 12 * (r // 4)
        db[r, at:at + 2] = -63.0
    db[37, 300] = -55.5                                 # the carrier's peak row
    return db


def test_detector_to_tracker_without_a_host_copy(X, torch_cuda):
    torch = torch_cuda
    detect = importlib.import_module("prgs-sdr-kspecanal_amd.detect")
    db = scene()
    assert dm.detect(db, 16, 4, 10.0)["total"] == 64 + 10 + 60 + 64                # the CPU model of the detector: no false alarm
    det = detect.SignalDetector(1024, 16, 4, 10.0, capacity=512)
    trk = X.EmissionTracker(1024, row_gap=0, bin_slop=1, capacity=64, max_spans=512)
    try:
        det.detect_rows_dev(torch.from_numpy(db).to("cuda:0"))
        trk.link_detector(det)                          # records and emissions_total stay on the device
        rec, total, comps = trk.tracks()
        labels = trk.labels()
        ev, ev_total = det.emissions()
        assert ev_total == len(ev) == 198 and len(labels) == 198
        agree((rec, total, comps, labels), tm.link(ev, 1024, 64, 0, 1, capacity=64))
        assert total == comps == 1 + 1 + 1 + 16         # carrier, burst, chirp, sixteen dwells
        carrier = rec[(rec["bin_lo"] == 299) & (rec["bin_hi"] == 301)]
        assert len(carrier) == 1
        c = carrier[0]
        assert (c["row_first"], c["row_last"], c["nspans"], c["flags"]) == (0, 63, 64, tm.FLAG_OPEN_END)
        assert (c["peak_row"], c["peak_bin"], c["peak_db"]) == (37, 300, np.float32(-55.5))
        burst = rec[rec["bin_lo"] == 600][0]
        assert (burst["row_first"], burst["row_last"], burst["cells"], burst["flags"]) == (20, 29, 80, 0)
        chirp = rec[rec["bin_lo"] == 702][0]
        assert (chirp["bin_hi"], chirp["nspans"], chirp["mid2_first"], chirp["mid2_last"]) == (761, 60, 1404, 1522)
        d = X.track_times_freqs(rec, np.arange(1024) * 1000.0, 0.001)
        assert abs(d["drift_hz_per_s"][list(rec["bin_lo"]).index(702)] - 1e6) < 1e-6           # one 1 kHz bin per 1 ms row
        assert sorted(rec["row_last"] - rec["row_first"] + 1)[:16] == [4] * 16
        # following the capture: more rows, a relink of the longer list
        det.detect_rows_dev(torch.from_numpy(db[:8].copy()).to("cuda:0"))
        trk.link_detector(det)
        ev, _ = det.emissions()
        agree(trk.tracks() + (trk.labels(),), tm.link(ev, 1024, 72, 0, 1, capacity=64))
        small = X.EmissionTracker(1024, max_spans=511)
        with pytest.raises(X.KsaError, match="holds 512 emissions, this tracker links at most max_spans = 511"):
            small.link_detector(det)                    # never a silent cut of the list
        small.close()
    finally:
        trk.close()
        det.close()


# ------------------------------------------------------------------------------------------ the command line
def test_cli_track_links_the_saved_emissions(X, torch_cuda, tmp_path, capsys):
    K = importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")
    n, frames = 512, 21
    common = ["zeroSpan", "fftSize", str(n), "window", "hanning", "source", "synth", "bPltLevels", "false", "bPltHeatMap", "false",
              "prgLoopCnt", str(frames), "frameBatch", "8", "detect", "16:2:8:mode=go:maxGap=3:events=300"]

    def run(extra):
        K.sdr_curscan = K._gpu_curscan
        capsys.readouterr()
        d = K.main(common + extra)
        return d, capsys.readouterr().out

    for front, decim in (([], 1), (["zoom", "4"], 4)):
        emis, save = tmp_path / ("e%d.npz" % decim), tmp_path / ("t%d.npz" % decim)
        d, out = run(front + ["track", "1:2:minRows=2:events=5", "trackSave", str(save), "detectSave", str(emis)])
        ev, z = np.load(emis)["emissions"], np.load(save)
        assert sorted(z.files) == ["bin_slop", "capacity", "center_hz", "components_total", "drift_hz_per_s", "duration_s", "labels",
                                   "min_rows", "min_spans", "row_gap", "row_period_s", "t_start_s", "tracks", "tracks_total",
                                   "width_hz"]
        want = tm.link(ev, n, frames, 1, 2, 2, 1, capacity=5)
        assert want[4] == 0 and want[1] >= 1 and len(ev) == int(np.load(emis)["emissions_total"]) >= frames
        assert tm.same_records(z["tracks"], want[0]) and (int(z["tracks_total"]), int(z["components_total"])) == want[1:3]
        assert np.array_equal(z["labels"], want[3]) and z["labels"].dtype == np.int32
        assert (int(z["row_gap"]), int(z["bin_slop"]), int(z["min_rows"]), int(z["min_spans"]), int(z["capacity"])) == (1, 2, 2, 1, 5)
        period = d["fullSize"] * decim / d["samplingRate"]                 # one frame at the rate the engine was fed
        assert float(z["row_period_s"]) == period
        derived = tm.times_freqs(want[0], d["freqs"], period)
        for k, v in derived.items():
            assert np.allclose(z[k], v, rtol=1e-12, atol=0), k
        assert tm.same_records(d["trackTracks"], want[0]) and (d["trackTotal"], d["trackComponents"]) == want[1:3]
        assert np.array_equal(d["trackLabels"], want[3])
        rows = want[0]["row_last"] - want[0]["row_first"] + 1
        assert ("INFO:zero_span: track emissions [%d], components [%d], tracks stored [%d] / total [%d], longest [%d] rows, "
                "open at the end [%d]" % (len(ev), want[2], len(want[0]), want[1], rows.max(),
                                          np.count_nonzero(want[0]["flags"] & 1))) in out
