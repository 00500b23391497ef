"""Host side of the scan survey (no GPU needed): survey.stitch_emissions against the brute-force model of survey_model.py on
seeded random lists, one hand-written case per rule of the contract (so that a model sharing a bug still fails), the refusals
that need no device, and the scanDetect / scanTrack keys of the command line."""
import importlib
import itertools

import numpy as np
import pytest

import survey_model as sm
from conftest import load_pkg

NBINS = 16


@pytest.fixture(scope="module")
def S():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.survey")


@pytest.fixture(scope="module")
def K():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")


def fields(rec):
    return [tuple(r) for r in rec[["row", "bin_lo", "bin_hi", "peak_bin", "ndet"]].tolist()]


# ------------------------------------------------------------------------------------------ the module
def test_the_module_is_exported_and_adds_no_binding(S):
    pkg = load_pkg()
    detect = importlib.import_module("prgs-sdr-kspecanal_amd.detect")
    track = importlib.import_module("prgs-sdr-kspecanal_amd.track")
    assert pkg.ScanSurvey is S.ScanSurvey and pkg.stitch_emissions is S.stitch_emissions
    assert {"ScanSurvey", "stitch_emissions"} <= set(pkg.__all__)
    assert S.EMISSION_DTYPE is detect.EMISSION_DTYPE and S.EMISSION_DTYPE == sm.EMISSION_DTYPE == track.SPAN_DTYPE
    assert S.COUNTERS == sm.COUNTERS
    assert not hasattr(S, "SIGNATURES") and not hasattr(S, "lib")       # it is a layer over detect and track, not a library


# ------------------------------------------------------------------------------------------ random lists against the model
GEOMETRY = [(steps, hop, total) for steps, hop in itertools.product((1, 2, 7), (8, 4, 16))
            for total in sorted({max(1, (steps - 1) * hop + 5), steps * hop, (steps - 1) * hop + NBINS})]


@pytest.mark.parametrize("steps,hop,total", GEOMETRY)
def test_random_lists_match_the_brute_force_model(S, steps, hop, total):
    """total: 5 elements into the last band (clipped inside it), steps x hop (what a scan has: at hop 8 the last band's second
    half is cut off) and everything the bands cover (nothing clipped)."""
    seen = {k: 0 for k in sm.COUNTERS}
    joined = 0
    for seed, (edge, dc) in enumerate(itertools.product((0, 1, NBINS // 2 - 1), repeat=2)):
        rec = sm.random_band_records(steps, hop, NBINS, npasses=4, seed=1000 * steps + 10 * hop + seed, empty_pass=2)
        assert len(rec) and 2 not in set((rec["row"] // steps).tolist())
        got, members, counters = S.stitch_emissions(rec, steps, hop, NBINS, total, edge=edge, dc=dc)
        want, want_members, want_counters = sm.stitch(rec, steps, hop, NBINS, total, edge=edge, dc=dc)
        assert sm.same_records(got, want), (edge, dc)
        assert members.dtype == np.int32 and np.array_equal(members, want_members), (edge, dc)
        assert counters == want_counters, (edge, dc)
        # what ktr_link demands of a list: ascending (row, bin_lo), disjoint within a row, inside the range
        assert np.all(got["bin_lo"] <= got["bin_hi"]) and np.all(got["bin_hi"] < total) and np.all(got["bin_lo"] >= 0)
        same_row = got["row"][1:] == got["row"][:-1]
        assert np.all((got["row"][1:] > got["row"][:-1]) | (same_row & (got["bin_lo"][1:] > got["bin_hi"][:-1] + 1)))
        assert np.all((got["bin_lo"] <= got["peak_bin"]) & (got["peak_bin"] <= got["bin_hi"]))
        assert int(members.sum()) + sum(counters.values()) == len(rec)
        for k in sm.COUNTERS:
            seen[k] += counters[k]
        joined += int(np.count_nonzero(members > 1))
    assert seen["dc_dropped"] > 0                                            # nothing above passes vacuously
    assert seen["clipped"] > 0 or total == (steps - 1) * hop + NBINS
    assert seen["edge_dropped"] > 0 or steps == 1 or hop == 16
    assert joined > 0 or steps == 1 or hop == 16


def test_an_empty_list_and_an_unsorted_one(S):
    got, members, counters = S.stitch_emissions(np.zeros(0, dtype=sm.EMISSION_DTYPE), 7, 8, NBINS, 56, edge=1, dc=1)
    assert got.dtype == sm.EMISSION_DTYPE and len(got) == 0 and members.dtype == np.int32 and len(members) == 0
    assert counters == dict(dc_dropped=0, edge_dropped=0, clipped=0)
    rec = sm.random_band_records(7, 8, NBINS, npasses=3, seed=5)
    want = sm.stitch(rec, 7, 8, NBINS, 56)
    shuffled = rec[np.random.default_rng(1).permutation(len(rec))]           # the order of the input does not matter
    got = S.stitch_emissions(shuffled, 7, 8, NBINS, 56)
    assert sm.same_records(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    with pytest.raises(S.KsaError, match="EMISSION_DTYPE"):
        S.stitch_emissions(np.zeros(3, dtype=np.int64), 7, 8, NBINS, 56)
    with pytest.raises(S.KsaError, match="hop 0"):
        S.stitch_emissions(rec, 7, 0, NBINS, 56)


# ------------------------------------------------------------------------------------------ one hand-written case per rule
def run(S, rows, steps=3, hop=8, total=24, **kw):
    """Both implementations on hand-written band records; the result of the function under test, checked against the model."""
    rec = sm.records_of(rows)
    got = S.stitch_emissions(rec, steps, hop, NBINS, total, **kw)
    want = sm.stitch(rec, steps, hop, NBINS, total, **kw)
    assert sm.same_records(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    return got


def test_rows_become_passes_and_bins_become_elements(S):
    got, members, counters = run(S, [(0, 2, 3), (1, 12, 12), (2, 5, 6), (4, 1, 1), (3 * 5 + 2, 0, 0)])
    assert fields(got) == [(0, 2, 3, 2, 2), (0, 20, 22, 20, 3), (1, 9, 9, 9, 1), (5, 16, 16, 16, 1)]
    assert members.tolist() == [1, 2, 1, 1] and sum(counters.values()) == 0          # 8 + 12 abuts 16 + 5 .. 16 + 6


def test_dc_drops_what_lies_around_the_band_centre(S):
    rows = [(0, 8, 8), (0, 7, 9), (0, 6, 9), (0, 7, 10), (1, 8, 8), (1, 0, 0)]
    got, _, counters = run(S, rows, dc=1)
    assert counters == dict(dc_dropped=3, edge_dropped=0, clipped=0)                  # 8..8 twice and 7..9: within 7 .. 9
    assert [r[1:3] for r in fields(got)] == [(6, 10)]                                # 6..9 and 7..10 of band 0, 8 + 0 of band 1
    got, _, counters = run(S, rows, dc=0)
    assert counters["dc_dropped"] == 0 and [r[1:3] for r in fields(got)] == [(6, 10), (16, 16)]
    got, _, counters = run(S, [(0, 1, 15), (0, 0, 15), (1, 1, 14)], dc=7)             # the widest dc: bins 1 .. 15
    assert counters["dc_dropped"] == 2 and [r[1:3] for r in fields(got)] == [(0, 15)]


def test_edge_drops_an_outer_peak_that_another_band_sees_inside(S):
    # band 1's bin 0 is element 8 = band 0's bin 8, an inner bin there: dropped.  Band 0's bin 0 is element 0, which no other
    # band covers: it stays, and so does band 2's bin 15, element 31 (total 32 here).
    got, _, counters = run(S, [(0, 0, 0), (1, 0, 0), (2, 15, 15), (1, 15, 15)], total=32, edge=1)
    assert counters == dict(dc_dropped=0, edge_dropped=2, clipped=0)                  # band 1's bin 15 is band 2's bin 7
    assert [r[1:3] for r in fields(got)] == [(0, 0), (31, 31)]
    # the peak decides, not the extent: 0..3 peaking at 2 stays with edge 2, peaking at 1 it goes
    got, _, counters = run(S, [(1, 0, 3, 2), (4, 0, 3, 1)], edge=2)
    assert counters["edge_dropped"] == 1 and fields(got) == [(0, 8, 11, 10, 4)]
    # covered only by another band's outer bins: it stays.  hop 12: band 1's bin 1 is element 13 = band 0's bin 13, and with
    # edge 3 the inner bins are 3 .. 12
    got, _, counters = run(S, [(1, 1, 1)], steps=2, hop=12, total=24, edge=3)
    assert counters["edge_dropped"] == 0 and [r[1:3] for r in fields(got)] == [(13, 13)]
    got, _, counters = run(S, [(1, 1, 1)], steps=2, hop=12, total=24, edge=2)         # edge 2: bin 13 is an inner bin of band 0
    assert counters["edge_dropped"] == 1 and len(got) == 0
    # the widest edge leaves bins 7 and 8 inside; a band that does not exist (s' = steps) covers nothing
    got, _, counters = run(S, [(0, 15, 15), (2, 9, 9)], steps=3, hop=8, total=32, edge=7)
    assert counters["edge_dropped"] == 1 and [r[1:3] for r in fields(got)] == [(25, 25)]   # 15 is band 1's bin 7; 25 would be band 3's
    # dc is judged first: a record both rules would drop counts once, as a dc drop
    _, _, counters = run(S, [(1, 7, 9, 8)], edge=7, dc=1)
    assert counters == dict(dc_dropped=1, edge_dropped=0, clipped=0)


def test_the_range_end_clips_extents_and_drops_peaks_beyond_it(S):
    got, _, counters = run(S, [(2, 4, 9, 7), (5, 4, 9, 8), (8, 8, 9, 8)])            # band 2 starts at 16, the range ends at 24
    assert counters == dict(dc_dropped=0, edge_dropped=0, clipped=2)                  # peaks at 24 are outside, 23 is the last inside
    assert fields(got) == [(0, 20, 23, 23, 4)]                                        # ndet 6 cut to the 4 elements left


def test_overlapping_abutting_and_nested_sightings_merge(S):
    rows = [(0, 4, 9, 5, -40.0, -91.0, 3), (1, 0, 2, 1, -30.0, -92.0, 2),           # 4..9 and 8..10: overlap
            (0, 12, 12, 12, -50.0), (1, 5, 5, 5, -50.0),                            # 12 and 13: abut
            (1, 8, 15, 9, -20.0, -93.0, 8), (2, 2, 3, 2, -60.0),                    # 16..23 holds 18..19: nested
            (0, 0, 0), (0, 2, 2)]                                                   # 0 and 2: one element between, not joined
    got, members, _ = run(S, rows)
    assert fields(got) == [(0, 0, 0, 0, 1), (0, 2, 2, 2, 1), (0, 4, 10, 9, 5), (0, 12, 13, 12, 2), (0, 16, 23, 17, 8)]
    assert members.tolist() == [1, 1, 2, 2, 2]
    assert got["peak_db"].tolist() == [-50.0, -50.0, -30.0, -50.0, -20.0] and got["floor_db"].tolist()[2] == -92.0
    # a chain: 0..5, 5..9 and 10..12 are one record although the first and the last are far apart
    got, members, _ = run(S, [(0, 0, 5), (0, 5, 9), (1, 2, 4)])
    assert fields(got) == [(0, 0, 12, 0, 13)] and members.tolist() == [3]
    # passes never merge, whatever their elements
    got, members, _ = run(S, [(0, 0, 5), (3, 0, 5), (4, 0, 0)])
    assert fields(got) == [(0, 0, 5, 0, 6), (1, 0, 5, 0, 6), (1, 8, 8, 8, 1)] and members.tolist() == [1, 1, 1]


def test_equal_peaks_go_to_the_lower_element_then_the_lower_band(S):
    got, _, _ = run(S, [(0, 8, 12, 12, -30.0, -91.0), (1, 0, 4, 2, -30.0, -92.0)])   # elements 12 and 10: band 1's is lower
    assert fields(got) == [(0, 8, 12, 10, 5)] and got["floor_db"].tolist() == [-92.0]
    got, _, _ = run(S, [(1, 0, 4, 2, -30.0, -92.0), (0, 8, 12, 10, -30.0, -91.0)])   # the same element from both: band 0 wins
    assert fields(got) == [(0, 8, 12, 10, 5)] and got["floor_db"].tolist() == [-91.0]
    got, _, _ = run(S, [(0, 8, 12, 8, -30.0, -91.0), (1, 0, 4, 4, -29.75, -92.0)])   # a greater peak beats a lower element
    assert fields(got) == [(0, 8, 12, 12, 5)] and got["peak_db"].tolist() == [-29.75]


def test_ndet_is_the_sum_capped_by_the_width(S):
    got, _, _ = run(S, [(0, 8, 15, 8, -50.0, -90.0, 3), (1, 0, 7, 0, -50.0, -90.0, 2)])
    assert fields(got) == [(0, 8, 15, 8, 5)]                                          # 3 + 2 detected bins of 8
    got, _, _ = run(S, [(0, 8, 15, 8, -50.0, -90.0, 8), (1, 0, 7, 0, -50.0, -90.0, 7)])
    assert fields(got) == [(0, 8, 15, 8, 8)]                                          # 15 would exceed the 8 elements


# ------------------------------------------------------------------------------------------ refusals that need no device
class NoEngine:
    """What ScanSurvey reads of an engine before it touches a device."""

    def __init__(self, fft_size=64, scan_total=256, scan_hop=32, max_frames=8, device=0):
        self.fft_size, self.scan_total, self.scan_hop, self.max_frames, self.device = fft_size, scan_total, scan_hop, max_frames, device
        self.calls = []

    def __getattr__(self, name):
        raise AssertionError("a refused survey touched the engine: %s" % name)


@pytest.mark.parametrize("engine,kw,text", [
    (dict(scan_total=0, scan_hop=0), {}, "an engine with scan geometry"),
    (dict(fft_size=32768, scan_total=4 * 32768, scan_hop=16384), {}, "fft_size 32768 is outside the detector's 16..16384"),
    ({}, dict(edge=32), "edge 32 is outside 0..31"),
    ({}, dict(edge=-1), "edge -1 is outside 0..31"),
    ({}, dict(dc=32), "dc 32 is outside 0..31"),
    ({}, dict(nsteps=7), "nsteps 7 is not the engine's pass length"),
    ({}, dict(nsteps=9), "nsteps 9 is not the engine's pass length"),
    (dict(max_frames=4), {}, "nsteps 8 is not the engine's pass length"),
    ({}, dict(cells=48), "cells 48 does not divide the stitched range of 256"),
    ({}, dict(cells=0), "cells 0 does not divide"),
    ({}, dict(capacity=0), "capacity 0 is outside"),
])
def test_the_survey_refuses_before_it_touches_anything(S, engine, kw, text):
    eng = NoEngine(**engine)
    args = dict(nsteps=8, train=8, guard=1, threshold_db=10.0)
    args.update(kw)
    with pytest.raises(S.KsaError) as e:
        S.ScanSurvey(eng, **args)
    assert text in str(e.value)


def test_every_refusal_has_its_own_text(S):
    texts = set()
    for engine, kw in ((dict(scan_total=0, scan_hop=0), {}), (dict(fft_size=32768, scan_total=4 * 32768, scan_hop=16384), {}),
                       ({}, dict(edge=40)), ({}, dict(nsteps=3)), ({}, dict(cells=48))):
        with pytest.raises(S.KsaError) as e:
            S.ScanSurvey(NoEngine(**engine), **dict(dict(nsteps=8, train=8, guard=1, threshold_db=10.0), **kw))
        texts.add(str(e.value))
    assert len(texts) == 5


# ------------------------------------------------------------------------------------------ command line
SCAN = ["scan", "startFreq", "100e6", "endFreq", "109.6e6", "fftSize", "64", "xRes", "64"]


def test_scan_keys_parse_in_each_form(K):
    d = K.handle_args({}, ["fmScan", "scanDetect", "32:2:10:dc=2", "scanTrack", "1:2:minRows=3"])
    assert d["survey.spec"] == dict(train=32, guard=2, threshold=10.0, mode="ca", min_width=1, max_gap=0, capacity=4096, edge=0, dc=2)
    assert d["surveyTrack.spec"] == dict(row_gap=1, bin_slop=2, min_rows=3, min_spans=1, capacity=4096)
    assert d["prgMode"] == "SCAN" and d["detect.spec"] is None and d["track.spec"] is None
    d = K.handle_args({}, SCAN + ["scanDetect", "8:0:6.5:MODE=GO:minWidth=3:maxGap=70:events=10:EDGE=31:dc=31", "scanDetectSave", "x.npz"])
    assert d["survey.spec"] == dict(train=8, guard=0, threshold=6.5, mode="go", min_width=3, max_gap=70, capacity=10, edge=31, dc=31)
    assert "surveyTrack.spec" not in d and d["scanDetectSave"] == "x.npz"
    d = K.handle_args({}, ["quickFullScan", "scanDetect", "8:1:6:edge=4", "scanTrack", "1024:16777216:events=1048576:minSpans=2",
                           "scanTrackSave", "y.npz"])
    assert d["survey.spec"]["edge"] == 4 and d["fftSize"] == 64
    assert d["surveyTrack.spec"] == dict(row_gap=1024, bin_slop=1 << 24, min_rows=1, min_spans=2, capacity=1 << 20)


def test_without_the_keys_nothing_is_left_behind(K, capsys):
    for argv in (["fmScan"], ["zeroSpan"], SCAN):
        d = K.handle_args({}, argv)
        assert "survey.spec" not in d and "surveyTrack.spec" not in d
        assert d["scanDetect"] == d["scanDetectSave"] == d["scanTrack"] == d["scanTrackSave"] == ""
    capsys.readouterr()
    d = K.handle_args({}, ["fmScan", "scanDetectSave", "x.npz", "scanTrackSave", "y.npz"])
    out = capsys.readouterr().out
    assert "WARN:handle_args: scanDetectSave [x.npz] is ignored without scanDetect" in out
    assert "WARN:handle_args: scanTrackSave [y.npz] is ignored without scanTrack" in out and "survey.spec" not in d
    d = {}
    K.handle_args(d, ["fmScan", "scanDetect", "8:1:6"])
    K.handle_args(d, ["fmScan"])                                  # the same dict, the key gone: so is the spec
    assert "survey.spec" not in d


@pytest.mark.parametrize("value", ["x", "32", "32:2", "32:2:", "0:2:10", "1025:2:10", "32:-1:10", "32:257:10", "32:2:-1", "32:2:101",
                                   "32:2:nan", "32:2:inf", "2.5:2:10", "32:2:10:mode=xx", "32:2:10:mode", "32:2:10:minWidth=0",
                                   "32:2:10:minWidth=65", "32:2:10:maxGap=-1", "32:2:10:maxGap=1025", "32:2:10:events=0",
                                   "32:2:10:events=1048577", "32:2:10:events=3:events=4", "32:2:10:minWidth=x", "32:2:10:12",
                                   "32:2:10:gap=3", "32:2:10:edge=-1", "32:2:10:edge=32", "32:2:10:dc=32", "32:2:10:dc=-1",
                                   "32:2:10:dc=1:dc=1", "32:2:10:edge=x", "32:2:10:dc"])
def test_scan_detect_refuses_with_the_rule(K, value, capsys):
    d = {}
    with pytest.raises(SystemExit):
        K.handle_args(d, SCAN + ["scanDetect", value])
    assert d["cmd.stop"] is True
    out = capsys.readouterr().out
    assert "ERROR:handle_args: scanDetect [%s]: " % value in out and K.SCAN_DETECT_RULE in out


@pytest.mark.parametrize("value", ["2", "x:1", "2:y", "-1:1", "1025:1", "2:-1", "2:16777217", "2:1:minRows=0", "2:1:minSpans=0",
                                   "2:1:minRows=2147483648", "2:1:events=0", "2:1:events=1048577", "2:1:bogus=1", "2:1:minRows",
                                   "2:1:events=4:events=5", "2:1:minRows=x"])
def test_scan_track_refuses_with_the_rule(K, value, capsys):
    d = {}
    with pytest.raises(SystemExit):
        K.handle_args(d, SCAN + ["scanDetect", "8:1:6", "scanTrack", value])
    assert d["cmd.stop"] is True
    out = capsys.readouterr().out
    assert "ERROR:handle_args: scanTrack [%s]: " % value in out and K.SCAN_TRACK_RULE in out


def test_the_scan_keys_are_scan_only_and_track_needs_detect(K, capsys):
    for mode in ("zeroSpan", "zeroSpanSave", "zeroSpanPlay"):
        for key, value in (("scanDetect", "8:1:6"), ("scanTrack", "1:2")):
            with pytest.raises(SystemExit):
                K.handle_args({}, [mode, "fftSize", "64", "xRes", "64", key, value])
            assert "ERROR:handle_args: %s [%s] is scan only, prgMode is [%s]" % (key, value, mode.upper()) in capsys.readouterr().out
    with pytest.raises(SystemExit):
        K.handle_args({}, ["zeroSpan", "scanDetect", "8:1"])                      # a malformed text is named first, as for detect
    assert K.SCAN_DETECT_RULE in capsys.readouterr().out
    with pytest.raises(SystemExit):
        K.handle_args({}, SCAN + ["scanTrack", "1:2"])
    assert ("ERROR:handle_args: scanTrack [1:2] links the emissions of scanDetect: give [scanDetect T:G:THR] as well"
            in capsys.readouterr().out)
    with pytest.raises(SystemExit):
        K.handle_args({}, ["fmScan", "fftSize", "32768", "scanDetect", "8:1:6"])  # a band row longer than the detector takes
    assert K.SCAN_DETECT_RULE in capsys.readouterr().out
    wide = ["scan", "startFreq", "30e6", "endFreq", "2.5e9", "fftSize", "16384", "scanDetect", "8:1:6"]
    assert K.handle_args({}, wide)["survey.spec"] is not None                     # about 1030 bands of 16384 bins: above 2^24
    with pytest.raises(SystemExit):
        K.handle_args({}, wide + ["scanTrack", "1:2"])
    out = capsys.readouterr().out
    assert "ERROR:handle_args: scanTrack [1:2]: the stitched range of [" in out and "] entries exceeds the linker's [16777216] bins" in out
    d = K.handle_args({}, ["scan", "startFreq", "30e6", "endFreq", "1.5e9", "fftSize", "16384", "scanDetect", "8:1:6", "scanTrack", "1:2"])
    assert d["surveyTrack.spec"] is not None                                       # quickFullScan's range at 16384: 613 bands fit


def test_the_zerospan_keys_still_refuse_a_scan_with_their_recorded_text(K, capsys):
    with pytest.raises(SystemExit):
        K.handle_args({}, ["fmScan", "detect", "8:2:6"])
    assert "ERROR:handle_args: detect [8:2:6] is zeroSpan only, prgMode is [SCAN]" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        K.handle_args({}, ["fmScan", "scanDetect", "8:1:6", "detect", "8:2:6", "track", "1:2"])
    assert "ERROR:handle_args: detect [8:2:6] is zeroSpan only, prgMode is [SCAN]" in capsys.readouterr().out
