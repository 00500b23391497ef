"""The scan survey on the GPU at the smallest shape at which stitching can go wrong: fftSize 64, scanRangeNonOverlap 0.5 (hop
32), a range of 4 sampling rates -- 256 stitched entries from 8 tuned bands, of which the last reaches 32 entries past the
range --, fullSize 256 (7 half-overlapping windows).  Element e of the range is the absolute frequency start + e x rate / 64;
band s tunes to element 32 s + 32 and sees the elements 32 s .. 32 s + 63 at its bins 0 .. 63.  The capture blocks are built
with numpy from tones on whole elements over weak noise:
  element 20    steady, in band 0 alone (the only elements one band covers)
  element 112   steady, in the overlap of bands 2 (bin 48) and 3 (bin 16)
  element 100   steady, bands 2 (bin 36) and 3 (bin 4, an outer bin once edge is 8)
  element 176   in passes 2 .. 4 of 6 only, bands 4 and 5
  element 272   steady, bin 48 of band 7: in the half of the last band that the range cuts off
  0 Hz          a constant in every block, the receiver's centre spike: bin 32 of every band and of no other band
Under the Hanning window a tone on a whole element fills exactly three bins.  Every list is compared with the integer models
(detect_model on the very float rows the survey detected on, then survey_model, then track_model) without a tolerance: every
decision downstream of the rows is an integer."""
import importlib

import numpy as np
import pytest

import detect_model as dm
import survey_model as sm
import track_model as tm
from conftest import load_pkg

pytestmark = pytest.mark.gpu

N, HOP, TOTAL, STEPS, FULL, PASSES = 64, 32, 256, 8, 256, 6
CFAR = dict(train=8, guard=2, threshold_db=10.0)
STEADY = {20: 0.2, 112: 0.15, 100: 0.1, 272: 0.2}               # element -> amplitude
BURST, BURST_AMP, BURST_PASSES = 176, 0.12, (2, 3, 4)
DC_AMP = 0.05
STATE_KEYS = ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg", "fftHM", "hm_index", "passes")


@pytest.fixture(scope="module")
def ksa():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return load_pkg()


@pytest.fixture(scope="module")
def K(ksa):
    return importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")


@pytest.fixture(scope="module")
def sources(ksa):
    return importlib.import_module("prgs-sdr-kspecanal_amd.sources")


def capture(npasses=PASSES, seed=2026):
    """complex64 [npasses][STEPS][FULL]: what a receiver tuned to band s would deliver in pass p."""
    rng = np.random.default_rng(seed)
    t = np.arange(FULL)
    x = (rng.standard_normal((npasses, STEPS, FULL)) + 1j * rng.standard_normal((npasses, STEPS, FULL))) * 0.002
    for p in range(npasses):
        tones = dict(STEADY)
        if p in BURST_PASSES:
            tones[BURST] = BURST_AMP
        for s in range(STEPS):
            x[p, s] += DC_AMP * np.exp(2j * np.pi * rng.random())
            for e, amp in tones.items():
                b = e - HOP * s
                if 0 <= b < N:
                    x[p, s] += amp * np.exp(2j * np.pi * ((b - N // 2) / N * t + rng.random()))
    return x.astype(np.complex64)


@pytest.fixture(scope="module")
def blocks():
    return capture()


def engine(ksa, raw=False):
    eng = ksa.SpectrumEngine(N, full_size=FULL, non_overlap=0.5, window="hanning", xres=64, max_frames=STEPS, device=0,
                             scan_total_entries=TOTAL, scan_non_overlap=0.5)
    eng.scan_set_base_is_raw(raw)
    return eng


def same_state(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in STATE_KEYS)


def run_survey(ksa, blocks, step_ok=None, **kw):
    """A survey over `blocks`: dict(rows = the band rows of every pass, per_pass = what scan_pass returned, emissions, members,
    total, counters, occupancy, passes, state); the survey and its engine are closed again."""
    eng = engine(ksa)
    sv = ksa.ScanSurvey(eng, STEPS, **dict(CFAR, cells=64, **kw))
    try:
        rows, per_pass = [], []
        for p in range(len(blocks)):
            per_pass.append(sv.scan_pass(blocks[p], step_ok=step_ok))
            rows.append(sv.band_rows().cpu().numpy().copy())
        ev, members, total = sv.emissions()
        return dict(rows=rows, per_pass=per_pass, emissions=ev, members=members, total=total, counters=dict(sv.counters),
                    occupancy=sv.occupancy(), passes=sv.passes, state=eng.scan_state(), band_lost=sv.band_lost)
    finally:
        sv.close()
        eng.close()


def model(rows, capacity=4096, edge=0, dc=0, mode="ca", min_width=1, max_gap=0):
    """detect_model over the band rows of every pass, then survey_model: (stitched, members, counters, band records)."""
    band = [dm.detect(r, CFAR["train"], CFAR["guard"], CFAR["threshold_db"], mode, min_width, max_gap, capacity=1 << 20,
                      row_base=p * STEPS)["all"] for p, r in enumerate(rows)]
    band = np.concatenate(band)
    stitched, members, counters = sm.stitch(band, STEPS, HOP, N, TOTAL, edge=edge, dc=dc)
    return stitched, members, counters, band


@pytest.fixture(scope="module")
def plain(ksa, blocks):
    return run_survey(ksa, blocks)


@pytest.fixture(scope="module")
def trimmed(ksa, blocks):
    return run_survey(ksa, blocks, edge=8, dc=1)


def holding(rec, row, element):
    """The indices of the records of `row` that hold `element`."""
    return np.flatnonzero((rec["row"] == row) & (rec["bin_lo"] <= element) & (element <= rec["bin_hi"]))


# ------------------------------------------------------------------------------------------ 1. the scan shows what it showed
@pytest.mark.parametrize("fmt,raw", [("c64", False), ("u8", False), ("s16", False), ("c64", True)])
def test_the_scan_state_is_what_scan_pass_leaves(ksa, sources, blocks, fmt, raw):
    x = blocks[:3]
    if fmt != "c64":
        x = np.stack([np.stack([sources.quantise(b.astype(np.complex128), fmt) for b in p]) for p in x])
        assert x.dtype == sources.IQ_FORMATS[fmt][0] and x.shape == (3, STEPS, 2 * FULL)
    ok = np.ones(STEPS, dtype=np.uint8)
    ok[5] = 0
    a, b = engine(ksa, raw), engine(ksa, raw)
    sv = ksa.ScanSurvey(b, STEPS, **CFAR)
    try:
        for p in range(3):
            a.scan_pass(x[p], step_ok=ok if p == 1 else None)
            sv.scan_pass(x[p], step_ok=ok if p == 1 else None)
            sa, sb = a.scan_state(), b.scan_state()
            assert same_state(sa, sb), (fmt, raw, p)
        assert sa["passes"] == 3 and sa["hm_index"] == 3 and np.isfinite(sa["Fft.Avg"]).all() and np.ptp(sa["Fft.Cur"]) > 20
    finally:
        sv.close()
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------ 2. the lists, exactly
@pytest.mark.parametrize("which,edge,dc", [("plain", 0, 0), ("trimmed", 8, 1)])
def test_the_lists_are_the_models_on_the_same_rows(request, which, edge, dc):
    got = request.getfixturevalue(which)
    stitched, members, counters, band = model(got["rows"], edge=edge, dc=dc)
    assert len(band) > len(stitched) > 0 and got["band_lost"] == 0
    assert sm.same_records(got["emissions"], stitched) and np.array_equal(got["members"], members)
    assert got["total"] == len(stitched) and got["counters"] == counters and got["passes"] == PASSES
    assert np.array_equal(got["occupancy"], sm.occupancy(stitched, PASSES, TOTAL, 64)) and got["occupancy"].dtype == np.int64
    for p in range(PASSES):
        assert sm.same_records(got["per_pass"][p], stitched[stitched["row"] == p]), p


# ------------------------------------------------------------------------------------------ 3. what the lists mean
def test_every_planted_tone_is_one_record_per_pass(plain):
    ev, members = plain["emissions"], plain["members"]
    for p in range(PASSES):
        for e, want in ((20, 1), (112, 2), (100, 2)):
            at = holding(ev, p, e)
            assert len(at) == 1 and members[at[0]] == want and ev["peak_bin"][at[0]] == e, (p, e)
            assert (ev["bin_lo"][at[0]], ev["bin_hi"][at[0]]) == (e - 1, e + 1), (p, e)
        at = holding(ev, p, BURST)
        assert len(at) == (1 if p in BURST_PASSES else 0), p
        if len(at):
            assert members[at[0]] == 2 and ev["peak_bin"][at[0]] == BURST
        for s in range(STEPS - 1):                            # the centre spike of bands 0 .. 6: one sighting each
            at = holding(ev, p, HOP * s + N // 2)
            assert len(at) == 1 and members[at[0]] == 1, (p, s)
    assert np.all(ev["bin_hi"] < TOTAL)
    # the cut-off tone and band 7's centre spike, element 256, were seen by band 7 and clipped, pass by pass
    band = model(plain["rows"])[3]
    last = band[band["row"] % STEPS == STEPS - 1]
    assert sorted(last["peak_bin"].tolist()) == sorted([N // 2, 272 - HOP * (STEPS - 1)] * PASSES)
    assert plain["counters"] == dict(dc_dropped=0, edge_dropped=0, clipped=2 * PASSES)
    assert plain["occupancy"][20 // 4] == PASSES and plain["occupancy"][BURST // 4] == len(BURST_PASSES)
    assert plain["occupancy"].max() == PASSES and plain["occupancy"][2] == 0


def test_dc_and_edge_trim_the_list(trimmed):
    ev, members = trimmed["emissions"], trimmed["members"]
    centres = HOP * np.arange(STEPS) + N // 2
    assert not any(len(holding(ev, p, c)) for p in range(PASSES) for c in centres)
    assert trimmed["counters"]["dc_dropped"] == STEPS * PASSES
    # element 100 is bin 4 of band 3, an outer bin at edge 8, and bin 36 of band 2: one sighting is left
    for p in range(PASSES):
        at = holding(ev, p, 100)
        assert len(at) == 1 and members[at[0]] == 1
        assert members[holding(ev, p, 112)[0]] == 2 and members[holding(ev, p, 20)[0]] == 1
    assert trimmed["counters"]["edge_dropped"] == PASSES and trimmed["counters"]["clipped"] == PASSES


def test_a_band_that_failed_to_tune_yields_nothing(ksa, blocks):
    ok = np.ones(STEPS, dtype=np.uint8)
    ok[2] = 0
    got = run_survey(ksa, blocks[:2], step_ok=ok)
    stitched, members, counters, band = model(got["rows"])
    assert sm.same_records(got["emissions"], stitched) and np.array_equal(got["members"], members) and got["counters"] == counters
    for p in range(2):
        assert np.ptp(got["rows"][p][2]) == 0 and np.ptp(got["rows"][p][3]) > 20          # the dummy band is flat
        assert not np.any(band["row"] == p * STEPS + 2)
        for e in (112, 100):                                  # band 3 alone sees them now
            at = holding(got["emissions"], p, e)
            assert len(at) == 1 and got["members"][at[0]] == 1
        assert len(holding(got["emissions"], p, 2 * HOP + N // 2)) == 0                     # band 2's own centre spike is gone


# ------------------------------------------------------------------------------------------ 4. tracks over the passes
def test_link_gives_one_track_per_tone(ksa, blocks, plain):
    eng = engine(ksa)
    sv = ksa.ScanSurvey(eng, STEPS, **CFAR)
    try:
        for p in range(PASSES):
            sv.scan_pass(blocks[p])
        spans = sv.emissions()[0]
        assert sm.same_records(spans, plain["emissions"])
        for params in (dict(row_gap=0, bin_slop=1), dict(row_gap=1, bin_slop=0, min_rows=4, min_spans=2, capacity=3)):
            tracks, total, comps, labels = sv.link(**params)
            want = tm.link(spans, TOTAL, PASSES, **params)
            assert want[4] == 0 and tm.same_records(tracks, want[0]) and (total, comps) == want[1:3], params
            assert labels.dtype == np.int32 and np.array_equal(labels, want[3]), params
        tracks, total, comps, labels = sv.link(row_gap=0, bin_slop=1)
        assert total == len(tracks) == comps
        steady = [20, 112, 100] + [HOP * s + N // 2 for s in range(STEPS - 1)]
        for e in steady:
            at = np.flatnonzero((tracks["bin_lo"] <= e) & (e <= tracks["bin_hi"]))
            assert len(at) == 1, e
            t = tracks[at[0]]
            assert (t["row_first"], t["row_last"], t["nspans"]) == (0, PASSES - 1, PASSES), e
            assert t["flags"] & tm.FLAG_OPEN_END
        at = np.flatnonzero((tracks["bin_lo"] <= BURST) & (BURST <= tracks["bin_hi"]))
        assert len(at) == 1
        t = tracks[at[0]]
        assert (t["row_first"], t["row_last"], t["nspans"], t["flags"]) == (2, 4, 3, 0)
        assert total == len(steady) + 1
    finally:
        sv.close()
        eng.close()


# ------------------------------------------------------------------------------------------ 5. capacity, lifetime, refusals
def test_capacity_two_stores_two_and_counts_all(ksa, blocks, plain):
    got = run_survey(ksa, blocks[:3], capacity=2)
    full = plain["emissions"][plain["emissions"]["row"] < 3]
    assert len(full) > 2 and got["total"] == len(full) and got["band_lost"] == 0
    assert sm.same_records(got["emissions"], full[:2]) and np.array_equal(got["members"], plain["members"][:2])
    assert np.array_equal(got["occupancy"], sm.occupancy(full, 3, TOTAL, 64))                # the cells count every record
    for p in range(3):
        assert sm.same_records(got["per_pass"][p], full[full["row"] == p])


def test_close_twice_and_the_refusals_leave_the_engine_alone(ksa, blocks):
    eng = engine(ksa)
    try:
        eng.scan_pass(blocks[0])
        before = eng.scan_state()
        for kw, text in ((dict(nsteps=7), "nsteps 7 is not the engine's pass length"), (dict(edge=32), "edge 32 is outside 0..31"),
                         (dict(dc=-1), "dc -1 is outside 0..31"), (dict(cells=48), "cells 48 does not divide the stitched range of 256"),
                         (dict(train=0), "train 0"), (dict(mode="xx"), "mode")):
            with pytest.raises(ksa.KsaError) as e:
                ksa.ScanSurvey(eng, **dict(dict(nsteps=STEPS, **CFAR), **kw))
            assert text in str(e.value), kw
        plain_eng = ksa.SpectrumEngine(N, full_size=FULL, non_overlap=0.5, window="hanning", xres=64, max_frames=STEPS, device=0)
        with pytest.raises(ksa.KsaError, match="an engine with scan geometry"):
            ksa.ScanSurvey(plain_eng, STEPS, **CFAR)
        plain_eng.close()
        sv = ksa.ScanSurvey(eng, STEPS, **CFAR)
        with pytest.raises(ksa.KsaError, match=r"scan_pass wants \[8\]\[256\]"):
            sv.scan_pass(blocks[0][:, :100])
        with pytest.raises(ksa.KsaError, match="step_ok has 3 entries for 8 steps"):
            sv.scan_pass(blocks[0], step_ok=np.ones(3, dtype=np.uint8))
        assert same_state(before, eng.scan_state()) and sv.passes == 0
        assert sv.link(0, 0)[1] == 0                          # no pass yet: an empty list links to nothing
        sv.close()
        sv.close()
        with pytest.raises(ksa.KsaError, match="the survey is closed"):
            sv.scan_pass(blocks[0])
        assert same_state(before, eng.scan_state())
        eng.scan_pass(blocks[1])                              # the engine is still the caller's and still works
        assert eng.scan_state()["passes"] == 2
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------ 6. the command line, end to end
def test_the_command_line_saves_what_a_survey_driven_by_hand_gives(ksa, K, tmp_path):
    keys = ["scan", "startFreq", "100e6", "endFreq", "109.6e6", "fftSize", "64", "xRes", "64", "window", "hanning", "source", "synth",
            "prgLoopCnt", "3", "scanDetect", "8:2:10:dc=1:edge=4", "scanTrack", "0:1:minRows=2", "bPltLevels", "false",
            "bPltHeatMap", "false"]
    det_file, trk_file = str(tmp_path / "survey.npz"), str(tmp_path / "tracks.npz")
    K.sdr_curscan = K._gpu_curscan
    d = K.main(keys + ["scanDetectSave", det_file, "scanTrackSave", trk_file])
    # by hand: the same source, tuned and read as scan_range does it, through a survey over an engine of the same geometry
    h = K.handle_args({}, keys)
    groups, total, centers = K.scan_geometry(h)
    assert (total, len(centers), h["fullSize"]) == (TOTAL, STEPS, 512)
    src = K.sources.SyntheticSdr()
    eng = K.get_engine(h, scan_total=total, max_frames=len(centers))
    sv = ksa.ScanSurvey(eng, len(centers), 8, 2, 10.0, dc=1, edge=4, cells=64)
    try:
        eng.scan_reset()
        for p in range(3):
            blk = np.empty((len(centers), h["fullSize"]), dtype=np.complex64)
            for s, fc in enumerate(centers):
                src, ok = K.sdr_setup(src, fc, h["samplingRate"], h["gain"])
                assert ok
                blk[s] = K.sdr_read(src, h["fullSize"])
            eng.set_flags(True, True, True)
            sv.scan_pass(blk)
        ev, members, n = sv.emissions()
        tracks, tracks_total, comps, labels = sv.link(0, 1, min_rows=2)
        state = eng.scan_state()
        assert len(ev) > 3 and len(tracks) > 0 and np.any(members == 2)
        z = np.load(det_file)
        assert sm.same_records(z["emissions"], ev) and np.array_equal(z["members"], members) and z["emissions_total"] == n
        assert np.array_equal(z["occupancy"], sv.occupancy()) and z["passes"] == 3
        assert {k: int(z[k]) for k in sm.COUNTERS} == sv.counters and sv.counters["dc_dropped"] > 0
        freqs = d["freqsAll"]
        step = (freqs[-1] - freqs[0]) / (TOTAL - 1)
        assert np.allclose(z["peak_hz"], freqs[ev["peak_bin"]], rtol=0, atol=1e-3)
        assert np.allclose(z["center_hz"], (freqs[ev["bin_lo"]] + freqs[ev["bin_hi"]]) / 2, rtol=0, atol=1e-3)
        assert np.allclose(z["width_hz"], (ev["bin_hi"] - ev["bin_lo"] + 1) * step, rtol=0, atol=1e-3)
        whole_mhz = np.abs(z["peak_hz"] / 1e6 - np.rint(z["peak_hz"] / 1e6)) * 1e6 <= 1.5 * step
        assert whole_mhz.all()                                # the synthetic source puts its tones on whole MHz, wherever it is tuned
        t = np.load(trk_file)
        assert tm.same_records(t["tracks"], tracks) and np.array_equal(t["labels"], labels)
        assert (t["tracks_total"], t["components_total"]) == (tracks_total, comps) and t["row_period_s"] > 0
        want = tm.times_freqs(tracks, freqs, float(t["row_period_s"]))
        for k in want:
            assert np.allclose(t[k], want[k], rtol=1e-12, atol=1e-6), k
        assert sm.same_records(d["surveyEmissions"], ev) and tm.same_records(d["surveyTracks"], tracks) and d["surveyPasses"] == 3
        for k in ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg"):   # and the scan itself shows what it shows without the keys
            assert np.array_equal(d[k], state[k]), k
    finally:
        sv.close()
        eng.close()
        h["ksa.engine"] = None
