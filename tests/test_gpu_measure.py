"""The band meter on the GPU against its float64 model (tests/measure_model.py).  mm.compare asserts, per record, first that the
model's margin makes the exact fields decidable (>= 1e-9) and then: every integer field and peak_db exactly, power, m1 and m2
within relative 1e-12, power_db within 2 float32 ulps.  Shapes are the smallest at which the kernel takes each of its paths:
windows of 1, 2, 63, 64, 65 bins, the wave / workgroup cut-over at 256 bins and one bin either side of it, the full row; rows
of 1, 16, 65, 4096 and 16385 bins; rows that allow 16-byte loads and rows that do not (a stride of nbins + 3, a base one float
off)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import measure_model as mm
from conftest import load_pkg

pytestmark = pytest.mark.gpu

CUT = mm.WAVE_MAX_BINS
WIDTHS = (1, 2, 63, 64, 65, CUT - 1, CUT, CUT + 1)
FLOOR, SIGMA = -90.0, 3.0
PAD = np.float32(400.0)                          # what lies between the rows of a strided buffer: a bin read from there shows


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def X():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.measure")


@pytest.fixture(scope="module")
def D():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.detect")


def make_rows(seed, nrows, nbins):
    """Seeded rows: a normal dB cloud with two carriers per row and, where the row is long enough, planted entries: NaN, -inf,
    +0 and -0 side by side (two equal peaks whose bits differ), +inf and 600 (two equal peaks after the clamp), -600, four NaN
    bins in a row (a window of invalid bins only) and two equal finite peaks ten bins apart."""
    rng = np.random.default_rng(seed)
    rows = (FLOOR + SIGMA * rng.standard_normal((nrows, nbins))).astype(np.float32)
    k = np.arange(nbins)
    for r in range(nrows):
        for c, w, top in ((0.3 + 0.02 * r, 0.004, 40.0), (0.7 - 0.01 * r, 0.02, 25.0)):
            rows[r] = np.maximum(rows[r], (FLOOR + top * np.exp(-0.5 * ((k / nbins - c) / w) ** 2)
                                           + 0.5 * rng.standard_normal(nbins)).astype(np.float32))
    if nbins >= 4096:
        rows[:, 300], rows[:, 301], rows[:, 310], rows[:, 311] = np.nan, -np.inf, 0.0, -0.0
        rows[:, 500], rows[:, 520], rows[:, 530] = np.inf, 600.0, -600.0
        rows[:, 40:44] = np.nan
        rows[:, 1000] = rows[:, 1010] = -20.0
    elif nbins >= 64:
        rows[:, 7], rows[:, 8], rows[:, 20], rows[:, 21] = np.nan, -np.inf, 0.0, -0.0
    elif nbins >= 16:
        rows[:, 5] = np.nan
    else:
        rows[:, 0] = [-50.0, np.nan, np.inf][:nrows] + [-60.0] * max(nrows - 3, 0)
    return rows


def bands_for(nbins):
    """Bands of every width of WIDTHS that fits, at an unaligned start, at the end of the row and at bin 0; the full row; the
    windows around the planted entries."""
    out = {(0, nbins - 1), (0, 0), (nbins - 1, nbins - 1)}
    for w in WIDTHS:
        for lo in (0, 2001 if nbins > 4000 else 1, nbins - w):
            if 0 <= lo and lo + w <= nbins:
                out.add((lo, lo + w - 1))
    if nbins >= 4096:
        out |= {(296, 320), (310, 311), (490, 540), (40, 43), (990, 1020), (38, 45)}
    elif nbins >= 64:
        out |= {(7, 8), (19, 22), (5, 24)}
    elif nbins >= 16:
        out |= {(5, 5), (3, 9)}
    return np.array(sorted(out), dtype=np.int32)


def on_device(torch, rows, stride=None, offset=0):
    """(tensor that owns the memory, address of row 0) of rows laid out `stride` floats apart, `offset` floats into the buffer."""
    nrows, nbins = rows.shape
    stride = nbins if stride is None else stride
    host = np.full(offset + nrows * stride + 4, PAD, dtype=np.float32)
    for r in range(nrows):
        host[offset + r * stride:offset + r * stride + nbins] = rows[r]
    buf = torch.from_numpy(host).to("cuda:0")
    return buf, buf.data_ptr() + 4 * offset


def span_list(torch, records):
    """(records tensor, count tensor) of 32-byte span records [(row, bin_lo, bin_hi)] in device memory, as the detector's."""
    ev = np.zeros(len(records), dtype=DETECT_DTYPE)
    for i, (row, lo, hi) in enumerate(records):
        ev[i]["row"], ev[i]["bin_lo"], ev[i]["bin_hi"] = row, lo, hi
    dev = torch.from_numpy(ev.view(np.uint8).copy()).to("cuda:0")
    return ev, dev


DETECT_DTYPE = np.dtype([("row", "<i8"), ("bin_lo", "<i4"), ("bin_hi", "<i4"), ("peak_bin", "<i4"), ("ndet", "<i4"),
                         ("peak_db", "<f4"), ("floor_db", "<f4")])


def total_dev(torch, n):
    return torch.tensor([n], dtype=torch.int64, device="cuda:0")


# ------------------------------------------------------------------------------------------ bands: every width, size and load form
LAYOUTS = {"tight": (0, 0), "stride+3": (3, 0), "offset1": (0, 1)}       # name -> (extra stride, offset in floats)


@pytest.fixture(scope="module")
def reference():
    """{nbins: (rows, bands, the model's results and margins)}: computed once, shared by the layouts, never written to."""
    out = {}
    for nbins in (1, 16, 65, 4096, 16385):
        rows = make_rows(100 + nbins, 3, nbins)
        bands = bands_for(nbins)
        want, margins = mm.measure_bands(rows, bands, 3 * len(bands), occupied=0.99, xdb=6.0, row_base=7)
        for a in (rows, bands, want, margins):
            a.setflags(write=False)
        out[nbins] = (rows, bands, want, margins)
    return out


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("nbins", [1, 16, 65, 4096, 16385])
def test_bands_match_the_model(X, torch, reference, nbins, layout):
    rows, bands, want, margins = reference[nbins]
    extra, offset = LAYOUTS[layout]
    buf, addr = on_device(torch, rows, nbins + extra, offset)
    m = X.SpectrumMeter(nbins, capacity=len(want), occupied=0.99, xdb=6.0)
    try:
        m.set_bands(bands)
        m.measure_bands_dev(addr, nrows=3, row_stride=nbins + extra, row_base=7)
        got = m.results()
        info = m.kernel_info()
    finally:
        m.close()
    mm.compare(got, want, margins, "nbins %d %s" % (nbins, layout))
    widths = bands[:, 1] - bands[:, 0] + 1
    assert info["vec"] == (1 if nbins % 4 == 0 and layout == "tight" else 0)
    assert info["form"] == (1 if widths.max() > CUT else 0) and info["threads"] == 256 and info["grid"] >= 1
    assert (want["flags"] & mm.FLAG_INVALID).any() and (want["nvalid"] == 0).any()          # every size has a window of invalid bins only


def test_the_host_rows_form_gives_the_same_bytes(X, torch, reference):
    rows, bands, want, margins = reference[4096]
    m = X.SpectrumMeter(4096, capacity=len(want), occupied=0.99, xdb=6.0)
    try:
        m.set_bands(bands)
        m.measure_bands(rows, row_base=7)
        got = m.results()
    finally:
        m.close()
    mm.compare(got, want, margins, "host rows")


@pytest.mark.parametrize("nb", [1, 3, 1024])
def test_bands_counts_slots_and_the_refusal_past_capacity(X, torch, nb):
    nbins, nrows, first_slot = 4096, 5, 11
    rows = make_rows(7 + nb, nrows, nbins)
    lo = (np.arange(nb) * 4) % (nbins - 400)
    bands = np.stack([lo, lo + (np.arange(nb) * 37) % 300], axis=1).astype(np.int32)     # widths 1 .. 300: both forms
    cap = first_slot + nrows * nb
    want, margins = mm.measure_bands(rows, bands, cap, occupied=0.9, xdb=10.0, row_base=0, first_slot=first_slot)
    buf, addr = on_device(torch, rows)
    m = X.SpectrumMeter(nbins, capacity=cap, occupied=0.9, xdb=10.0)
    try:
        m.set_bands(bands)
        m.measure_bands_dev(addr, nrows=nrows, first_slot=first_slot)
        got = m.results()
        mm.compare(got[first_slot:], want[first_slot:], margins[first_slot:], "%d bands" % nb)
        assert not got[:first_slot].view(np.uint8).any()
        for bad in (first_slot + 1, cap):
            with pytest.raises(X.KsaError, match="capacity"):
                m.measure_bands_dev(addr, nrows=nrows, first_slot=bad)
        with pytest.raises(X.KsaError, match="capacity"):
            m.measure_bands_dev(addr, nrows=nrows + 1, first_slot=first_slot)
        with pytest.raises(X.KsaError, match="first_slot"):
            m.measure_bands_dev(addr, nrows=nrows, first_slot=-1)
        for b, text in (([[0, nbins]], "band 0"), ([[5, 4]], "band 0"), ([[0, 1], [-1, 3]], "band 1"), (np.zeros((1025, 2)), "nb 1025")):
            with pytest.raises(X.KsaError, match=text):
                m.set_bands(b)
        assert m.results().tobytes() == got.tobytes() and np.array_equal(m.bands, bands)      # refusals leave everything as it was
        m.set_bands(np.zeros((0, 2), dtype=np.int32))
        m.measure_bands_dev(addr, nrows=nrows, first_slot=cap)                                # no band: nothing to do, nothing refused
        assert m.results().tobytes() == got.tobytes()
    finally:
        m.close()


# ------------------------------------------------------------------------------------------ spans
NB, NR = 4096, 12


@pytest.fixture(scope="module")
def span_rows():
    a, b = make_rows(31, 30, NB), make_rows(32, 8, NB)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def test_spans_margin_clipping_and_slots_outside_the_batch_stay(X, torch, span_rows):
    rows_a, rows_b = span_rows                   # rows 90 .. 119 for the call that fills every slot, rows 100 .. 107 for the second
    records = [(95, 100, 140), (99, 2, 30), (100, 2, 30), (100, 1200, 1449), (101, NB - 30, NB - 3), (102, 0, NB - 1),
               (103, 50, 40), (103, -1, 10), (103, 10, NB), (104, 3, 3), (105, 1000, 1010), (107, 2001, 2001 + CUT - 11),
               (107, 2001, 2001 + CUT - 10), (108, 100, 140), (119, 5, 9)]
    ev, dev = span_list(torch, records)
    cap, margin = 20, 5
    first_want, first_margins = mm.measure_spans(rows_a, ev, len(ev), cap, 0.99, 3.0, margin, row_base=90)
    want, margins = mm.measure_spans(rows_b, ev, len(ev), cap, 0.99, 3.0, margin, row_base=100, before=first_want)
    m = X.SpectrumMeter(NB, capacity=cap, occupied=0.99, xdb=3.0, margin=margin)
    try:
        buf_a, addr_a = on_device(torch, rows_a)
        buf_b, addr_b = on_device(torch, rows_b)
        m.measure_spans_dev(addr_a, dev, total_dev(torch, len(ev)), nrows=30, row_base=90, span_capacity=len(ev))
        got_a = m.results()
        m.measure_spans_dev(addr_b, dev, total_dev(torch, len(ev)), nrows=8, row_base=100, span_capacity=len(ev))
        got = m.results()
    finally:
        m.close()
    mm.compare(got_a, first_want, np.where(np.isinf(first_margins), 1.0, first_margins), "first call")
    touched = ~np.isinf(margins)
    assert touched.sum() == 8 and list(np.flatnonzero(~touched)[:5]) == [0, 1, 6, 7, 8]
    mm.compare(got[touched], want[touched], margins[touched], "second call")
    assert got[~touched].tobytes() == got_a[~touched].tobytes()                  # rows before and after the batch, malformed spans
    assert not got[[6, 7, 8]].view(np.uint8).any() and not got[len(ev):].view(np.uint8).any()
    clipped = (want["flags"] & mm.FLAG_CLIPPED) != 0
    assert list(np.flatnonzero(clipped)) == [1, 2, 4, 5, 9] and (want["bin_lo"][2], want["bin_hi"][4]) == (0, NB - 1)
    assert (want["bin_hi"][11] - want["bin_lo"][11] + 1, want["bin_hi"][12] - want["bin_lo"][12] + 1) == (CUT, CUT + 1)


def test_spans_first_total_and_capacity_bound_the_slots(X, torch, span_rows):
    rows = span_rows[1]
    records = [(100 + i % 8, 10 * i, 10 * i + 3 + i) for i in range(40)]
    ev, dev = span_list(torch, records)
    buf, addr = on_device(torch, rows)
    m = X.SpectrumMeter(NB, capacity=32, occupied=0.99, xdb=3.0)
    try:
        call = lambda total, first, span_cap=40: m.measure_spans_dev(addr, dev, total_dev(torch, total), nrows=8, row_base=100,
                                                                     span_capacity=span_cap, first=first)
        call(25, 25)                                          # first at the total
        call(25, 31)                                          # and beyond it
        call(0, 0)
        assert not m.results().view(np.uint8).any()
        call(25, 20)
        got = m.results()
        want, margins = mm.measure_spans(rows, ev, 25, 32, row_base=100, first=20)
        mm.compare(got[20:25], want[20:25], margins[20:25], "first 20 of 25")
        assert not got[:20].view(np.uint8).any() and not got[25:].view(np.uint8).any()
        call(10 ** 6, 0)                                      # a total beyond the list and beyond the capacity
        want, margins = mm.measure_spans(rows, ev, 10 ** 6, 32, row_base=100)
        mm.compare(m.results(), want, margins, "total beyond capacity")
        m.reset()
        call(10 ** 6, 0, 7)                                   # the list's own room bounds it too
        got = m.results()
        mm.compare(got[:7], want[:7], margins[:7], "span_capacity 7")
        assert not got[7:].view(np.uint8).any()
    finally:
        m.close()


def test_spans_of_a_real_detector_pair_by_index(X, D, torch, span_rows):
    rows = span_rows[0][:NR]
    buf, addr = on_device(torch, rows)
    det = D.SignalDetector(NB, 32, 4, 8.0, mode="ca", min_width=2, max_gap=3, capacity=1024)
    # a margin that carries the narrow emissions (a few bins) to the wave form and the carriers (some 30 bins) past the cut-over
    m = X.SpectrumMeter(NB, capacity=1024, occupied=0.99, xdb=6.0, margin=116)
    host = X.SpectrumMeter(NB, capacity=1024, occupied=0.99, xdb=6.0, margin=116)
    try:
        det.detect_rows_dev(addr, nrows=NR)
        m.measure_detector(det, addr, row_base=0, nrows=NR)   # the records and their count are read where the detector left them
        ev, total = det.emissions()
        got = m.results()
        host.measure_detector(det, rows[:5], row_base=0)      # the host-rows form, in two calls
        host.measure_detector(det, rows[5:], row_base=5, first=int(np.searchsorted(ev["row"], 5)))
        assert host.results().tobytes() == got.tobytes()
    finally:
        m.close()
        host.close()
        det.close()
    assert 10 <= len(ev) == total <= 1024
    want, margins = mm.measure_spans(rows, ev, total, 1024, 0.99, 6.0, 116)
    mm.compare(got[:len(ev)], want[:len(ev)], margins[:len(ev)], "detector")
    assert np.array_equal(got["row"][:len(ev)], ev["row"]) and np.all(got["bin_lo"][:len(ev)] <= ev["bin_lo"])
    widths = got["bin_hi"][:len(ev)] - got["bin_lo"][:len(ev)] + 1
    assert widths.min() <= CUT < widths.max() and not got[len(ev):].view(np.uint8).any()


# ------------------------------------------------------------------------------------------ calls, parameters, streams
def test_one_call_over_21_rows_equals_three_calls(X, torch):
    rows = make_rows(5, 21, NB)
    bands = np.array([[0, 99], [2001, 2001 + CUT], [310, 311]], dtype=np.int32)
    records = [(r, 100 + 7 * r, 130 + 20 * r) for r in range(21)]
    ev, dev = span_list(torch, records)
    buf, addr = on_device(torch, rows)
    one, three = (X.SpectrumMeter(NB, capacity=128) for _ in range(2))
    try:
        for m in (one, three):
            m.set_bands(bands)
        one.measure_spans_dev(addr, dev, total_dev(torch, 21), nrows=21, row_base=0, span_capacity=21, first=0)
        one.measure_bands_dev(addr, nrows=21, first_slot=64)
        for start, n in ((0, 8), (8, 8), (16, 5)):
            three.measure_bands_dev(addr + 4 * NB * start, nrows=n, row_base=start, first_slot=64 + 3 * start)
            three.measure_spans_dev(addr + 4 * NB * start, dev, total_dev(torch, 21), nrows=n, row_base=start, span_capacity=21)
        a, b = one.results(), three.results()
    finally:
        one.close()
        three.close()
    assert a.tobytes() == b.tobytes() and (a["flags"][:21] & 1).all() and (a["flags"][64:127] & 1).all()
    want, margins = mm.measure_spans(rows, ev, 21, 21)
    mm.compare(a[:21], want, margins, "21 rows of spans")
    want, margins = mm.measure_bands(rows, bands, 63)
    mm.compare(a[64:127], want, margins, "21 rows of bands")


def test_set_params_holds_from_the_next_call_and_reset_zeroes(X, torch):
    rows = make_rows(9, 2, NB)
    bands = np.array([[1150, 1330], [2600, 3100]], dtype=np.int32)
    buf, addr = on_device(torch, rows)
    m = X.SpectrumMeter(NB, capacity=8, occupied=0.99, xdb=3.0)
    try:
        m.set_bands(bands)
        m.measure_bands_dev(addr, nrows=2, first_slot=0)
        m.set_params(occupied=0.5, xdb=20.0)                  # enqueued work keeps the old values
        m.measure_bands_dev(addr, nrows=2, first_slot=4)
        got = m.results()
        for bad, text in ((dict(occupied=1.0), "occupied"), (dict(occupied=0.49), "occupied"), (dict(xdb=-1.0), "xdb"),
                          (dict(xdb=float("inf")), "xdb"), (dict(margin=65537), "margin"), (dict(margin=-1), "margin")):
            with pytest.raises(X.KsaError, match=text):
                m.set_params(**bad)
        assert m.params == (0.5, 20.0, 0)
        m.reset()
        assert not m.results().view(np.uint8).any()
    finally:
        m.close()
    old, m_old = mm.measure_bands(rows, bands, 4, 0.99, 3.0)
    new, m_new = mm.measure_bands(rows, bands, 4, 0.5, 20.0)
    mm.compare(got[:4], old, m_old, "before set_params")
    mm.compare(got[4:], new, m_new, "after set_params")
    assert (new["obw_hi"] - new["obw_lo"] < old["obw_hi"] - old["obw_lo"]).all() and (new["xdb_hi"] - new["xdb_lo"] > old["xdb_hi"] - old["xdb_lo"]).all()


def test_two_objects_interleaved_on_two_streams(X, torch):
    rows = [make_rows(40 + i, 4, NB) for i in range(2)]
    bands = [np.array([[0, NB - 1], [100, 163]], dtype=np.int32), np.array([[2001, 2300], [5, 5], [990, 1020]], dtype=np.int32)]
    streams = [torch.cuda.Stream(device="cuda:0") for _ in range(2)]
    devs = [on_device(torch, r) for r in rows]
    torch.cuda.synchronize()
    meters = [X.SpectrumMeter(NB, capacity=64, occupied=0.95, xdb=6.0, stream=s.cuda_stream) for s in streams]
    try:
        for m, b in zip(meters, bands):
            m.set_bands(b)
        for r in range(4):                                    # a row at a time, the two objects in turn
            for m, b, (_, addr) in zip(meters, bands, devs):
                m.measure_bands_dev(addr + 4 * NB * r, nrows=1, row_base=r, first_slot=len(b) * r)
        got = [m.results() for m in meters]
    finally:
        for m in meters:
            m.close()
    for g, r, b in zip(got, rows, bands):
        want, margins = mm.measure_bands(r, b, 64, 0.95, 6.0)
        mm.compare(g[:4 * len(b)], want[:4 * len(b)], margins[:4 * len(b)], "stream")
        assert not g[4 * len(b):].view(np.uint8).any()


def test_every_refusal_of_a_call_leaves_the_results_as_they_were(X, torch, span_rows):
    rows = span_rows[1]
    ev, dev = span_list(torch, [(100, 10, 20)])
    buf, addr = on_device(torch, rows)
    tot = total_dev(torch, 1)
    m = X.SpectrumMeter(NB, capacity=4)
    try:
        m.set_bands([[0, 9]])
        m.measure_spans_dev(addr, dev, tot, nrows=8, row_base=100, span_capacity=1)
        before = m.results()
        assert before["flags"][0] == 1
        h, L, p = m._h, X.lib(), C.c_void_p
        sp, tp, ra = p(dev.data_ptr()), p(tot.data_ptr()), p(addr)
        spans = lambda **k: L.kme_measure_spans_dev(h, k.get("rows", ra), k.get("stride", NB), k.get("nrows", 8), k.get("base", 100),
                                                    k.get("spans", sp), k.get("ss", 32), k.get("total", tp), k.get("cap", 1), k.get("first", 0))
        for kw, text in ((dict(rows=None), "null rows"), (dict(spans=None), "null spans"), (dict(total=None), "null span total"),
                         (dict(nrows=-1), "nrows -1"), (dict(stride=NB - 1), "row_stride"), (dict(ss=8), "span stride 8"),
                         (dict(ss=20), "span stride 20"), (dict(first=-1), "first -1"), (dict(base=-1), "row base -1"),
                         (dict(cap=-1), "span_capacity -1"), (dict(rows=p(addr + 2)), "4-byte aligned")):
            assert spans(**kw) != 0 and text in L.kme_last_error().decode(), kw
        host = np.zeros((1, NB), dtype=np.float32)
        assert L.kme_measure_spans(h, None, 1, 0, sp, 32, tp, 1, 0) != 0 and "null rows" in L.kme_last_error().decode()
        assert L.kme_measure_spans(h, host.ctypes.data_as(p), 1, 0, sp, 12, tp, 1, 0) != 0 and "span stride" in L.kme_last_error().decode()
        assert L.kme_measure_bands_dev(h, ra, NB, -1, 0, 0) != 0 and "nrows -1" in L.kme_last_error().decode()
        assert L.kme_measure_bands_dev(h, ra, NB - 1, 1, 0, 0) != 0 and "row_stride" in L.kme_last_error().decode()
        assert L.kme_measure_bands_dev(h, ra, NB, 1, -1, 0) != 0 and "row base" in L.kme_last_error().decode()
        assert L.kme_measure_bands(h, None, 1, 0, 0) != 0 and "null rows" in L.kme_last_error().decode()
        assert L.kme_read_results(h, None, 0, 1) != 0 and "null results" in L.kme_last_error().decode()
        assert L.kme_read_results(h, None, -1, 0) != 0 and L.kme_read_results(h, None, 0, -1) != 0
        assert L.kme_read_results(h, None, 3, 2) != 0 and "capacity" in L.kme_last_error().decode()
        assert L.kme_results_dev(h, None) != 0 and "null out" in L.kme_last_error().decode()
        assert m.results().tobytes() == before.tobytes()
        view = m.results_view()
        assert view.__cuda_array_interface__["shape"] == (4, 80) and view.__cuda_array_interface__["data"][0] != 0
    finally:
        m.close()


# ------------------------------------------------------------------------------------------ the command line
N, FRAMES, RATE = 64, 21, 2048000
SETTLE = 16 * 1024                                           # the samples sdr_setup discards


def two_carrier_capture(full):
    per_read = int(2 ** np.ceil(np.log2(full)))
    rng = np.random.default_rng(77)
    n = FRAMES * per_read
    t = np.arange(n)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.003
    x += 0.3 * np.exp(2j * np.pi * (-0.25 + 0.004 * np.sin(2 * np.pi * t / 900)) * t)       # a carrier with a little FM
    x += 0.1 * np.exp(2j * np.pi * 0.19 * t) * (1 + 0.5 * np.sin(2 * np.pi * t / 37))       # a weaker one with AM
    iq = np.zeros((SETTLE + n, 2), dtype=np.int16)
    iq[SETTLE:, 0], iq[SETTLE:, 1] = np.rint(x.real * 16384), np.rint(x.imag * 16384)
    return iq


def test_cli_measure_saves_what_the_model_gives_and_leaves_detect_alone(torch, X, tmp_path, monkeypatch):
    load_pkg()
    K = importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")
    common = ["zeroSpan", "fftSize", str(N), "xRes", str(N), "samplingRate", str(RATE), "iqFormat", "s16", "window", "hanning",
              "frameBatch", "8", "bPltLevels", "false", "bPltHeatMap", "false", "prgLoopCnt", str(FRAMES)]
    two_carrier_capture(K.handle_args({}, common)["fullSize"]).tofile(tmp_path / "capture.s16")
    common += ["source", "file:%s" % (tmp_path / "capture.s16"), "detect", "8:2:6"]
    fed = []
    feed = K._DetectFeed.feed_rows
    monkeypatch.setattr(K._DetectFeed, "feed_rows", lambda self, db: (fed.append(np.array(db, dtype=np.float32)), feed(self, db))[1])
    K.sdr_curscan = K._gpu_curscan
    plain = K.main(common + ["detectSave", str(tmp_path / "plain.npz")])
    assert "measureResults" not in plain and not [k for k in plain if k.startswith("measure") and k not in ("measure", "measureSave")]
    rows = np.concatenate(fed)
    del fed[:]
    K.sdr_curscan = K._gpu_curscan
    d = K.main(common + ["detectSave", str(tmp_path / "with.npz"), "measure", "99:xdb=6:margin=2", "measureSave", str(tmp_path / "m.npz")])
    assert np.array_equal(np.concatenate(fed), rows) and rows.shape == (FRAMES, N)
    a, b = np.load(tmp_path / "plain.npz"), np.load(tmp_path / "with.npz")
    assert sorted(a.files) == sorted(b.files) and all(a[k].tobytes() == b[k].tobytes() and a[k].dtype == b[k].dtype for k in a.files)
    ev = d["detectEmissions"]
    assert len(ev) >= FRAMES and d["measure.plan"] == dict(percent=99.0, occupied=float(np.float32(0.99)), xdb=6.0, margin=2)
    want, margins = mm.measure_spans(rows, ev, len(ev), len(ev), d["measure.plan"]["occupied"], 6.0, 2)
    z = np.load(tmp_path / "m.npz")
    mm.compare(z["results"], want, margins, "measureSave")
    assert z["results"].tobytes() == d["measureResults"].tobytes() and z["results"].dtype == X.RESULT_DTYPE
    assert (float(z["occupied_percent"]), float(z["xdb"]), int(z["margin"])) == (99.0, 6.0, 2) and z["occupied"] == np.float32(0.99)
    step = RATE / N
    f0 = d["freqs"][0]
    assert np.allclose(z["center_hz"], f0 + (want["bin_lo"] + want["m1"] / want["power"]) * step, rtol=0, atol=1e-6 * step)
    assert np.allclose(z["obw_hz"], (want["obw_hi"] - want["obw_lo"] + 1) * step, rtol=1e-12, atol=0)
    assert np.allclose(z["xdb_hz"], (want["xdb_hi"] - want["xdb_lo"] + 1) * step, rtol=1e-12, atol=0)
    noise = (want["bin_hi"] - want["bin_lo"] + 1) * 10.0 ** (ev["floor_db"].astype(np.float64) / 10)
    net = want["power"] - noise
    assert np.array_equal(np.isnan(z["power_net_db"]), ~(net > 0)) and (net > 0).any()
    ok = net > 0
    assert np.allclose(z["power_net_db"][ok], 10 * np.log10(net[ok]), rtol=0, atol=1e-6)
    assert np.allclose(z["snr_db"][ok], 10 * np.log10(net[ok] / noise[ok]), rtol=0, atol=1e-6)
