"""Scan survey: the emissions of a scan, listed per pass over the stitched range and linked into tracks.  A scan tunes
`steps` overlapping bands per pass; the engine leaves every band's dB row on the device (scan_spectra_dev) and stitches the pass
from those rows (scan_stitch_dev).  ScanSurvey runs the CFAR detector of detect.py over the same rows, band by band -- each
band has its own gain and floor, and CFAR has no wrap-around --, maps every band record to elements of the stitched range, joins
the sightings that overlapping bands give of one emission (stitch_emissions, numpy, every decision an integer but one float
compare) and hands one ordered, disjoint list per pass to the linker of track.py, whose rows are then the passes.  The hot path
is the HIP that is already there: spectra, CFAR and linking; this module adds no kernel.  There is no fallback: a missing
library raises."""
import numpy as np

from . import detect as _detect
from . import track as _track
from ._lib import KsaError, FMT_C64, FMT_U8, FMT_S8, FMT_S16
from .detect import EMISSION_DTYPE, SignalDetector
from .track import EmissionTracker

COUNTERS = ("dc_dropped", "edge_dropped", "clipped")


def stitch_emissions(records, steps, hop, nbins, total, edge=0, dc=0):
    """Band records -> (stitched, members, counters).  records: detect.EMISSION_DTYPE whose row is pass * steps + s, s the band
    of the pass, as the detector numbers the rows of a pass; band s covers the elements s * hop .. s * hop + nbins - 1 of the
    stitched range of `total` entries.  stitched: the same dtype (the bytes of track.SPAN_DTYPE), row = the pass, the bins
    elements e = s * hop + bin, ascending in (row, bin_lo) and disjoint within a row; members: int32, the band sightings joined
    into each record; counters: dict of the three drop counts.  In order:
    1. dc = K > 0: a band record with nbins/2 - K <= bin_lo and bin_hi <= nbins/2 + K is dropped (the receiver's centre spike,
       which a scan has once per tuned band): dc_dropped.
    2. edge = K > 0: a band record whose peak_bin lies in the outer K bins (< K or >= nbins - K) is dropped if another band
       s' of 0 .. steps - 1 covers the peak's element at a bin inside [K, nbins - K); otherwise it stays, so the two ends of the
       range lose nothing: edge_dropped.
    3. A record whose peak element is >= total is dropped (the last bands reach past the range): clipped; otherwise bin_hi is
       clipped to total - 1.
    4. Within a pass the survivors are sorted by (lo, hi, s); a record joins the current group when lo <= group_hi + 1, so
       overlapping and abutting records merge as the detector itself treats adjacent bins.  bin_lo is the least lo, bin_hi the
       greatest hi; peak_bin, peak_db and floor_db are those of the member with the greatest peak_db (ties: the lower element,
       then the lower band); ndet = min(sum of ndet, bin_hi - bin_lo + 1)."""
    rec = np.ascontiguousarray(records)
    if rec.dtype.itemsize != EMISSION_DTYPE.itemsize or rec.dtype.names != EMISSION_DTYPE.names:
        raise KsaError("stitch_emissions wants records of EMISSION_DTYPE (32 bytes), got %s" % (rec.dtype,))
    steps, hop, nbins, total, edge, dc = int(steps), int(hop), int(nbins), int(total), int(edge), int(dc)
    if steps < 1 or hop < 1 or nbins < 1 or total < 1 or edge < 0 or dc < 0:
        raise KsaError("stitch_emissions: steps %d, hop %d, nbins %d and total %d must be >= 1, edge %d and dc %d >= 0"
                       % (steps, hop, nbins, total, edge, dc))
    rec = rec.reshape(-1)
    counters = dict.fromkeys(COUNTERS, 0)
    row = rec["row"].astype(np.int64)
    npass, band = row // steps, row % steps
    lo, hi, pk = (rec[k].astype(np.int64) for k in ("bin_lo", "bin_hi", "peak_bin"))
    keep = np.ones(len(rec), dtype=bool)
    if dc > 0:
        drop = (nbins // 2 - dc <= lo) & (hi <= nbins // 2 + dc)
        counters["dc_dropped"] = int(np.count_nonzero(drop))
        keep &= ~drop
    off = band * hop
    e_pk = off + pk
    if edge > 0:
        # the bands s' whose bin e_pk - s' * hop lies in [edge, nbins - edge): s' * hop in (e_pk - nbins + edge, e_pk - edge].
        # The record's own band is never one of them: there the bin is peak_bin, an outer one.
        first = np.maximum(-((nbins - edge - 1 - e_pk) // hop), 0)           # ceil((e_pk - nbins + edge + 1) / hop)
        last = np.minimum((e_pk - edge) // hop, steps - 1)
        drop = keep & ((pk < edge) | (pk >= nbins - edge)) & (first <= last)
        counters["edge_dropped"] = int(np.count_nonzero(drop))
        keep &= ~drop
    drop = keep & (e_pk >= total)
    counters["clipped"] = int(np.count_nonzero(drop))
    keep &= ~drop
    at = np.flatnonzero(keep)
    if not len(at):
        return np.zeros(0, dtype=EMISSION_DTYPE), np.zeros(0, dtype=np.int32), counters
    npass, band, e_pk = npass[at], band[at], e_pk[at]
    e_lo, e_hi = off[at] + lo[at], np.minimum(off[at] + hi[at], total - 1)
    order = np.lexsort((band, e_hi, e_lo, npass))
    at, npass, band, e_pk, e_lo, e_hi = at[order], npass[order], band[order], e_pk[order], e_lo[order], e_hi[order]
    # one sweep for all passes: pass p lives at p * big + element, so the running greatest hi of a pass lies below every lo
    # of the next by more than the 1 that still joins
    big = total + 2
    reach = np.maximum.accumulate(npass * big + e_hi)
    new = np.ones(len(at), dtype=bool)
    new[1:] = npass[1:] * big + e_lo[1:] > reach[:-1] + 1
    start = np.flatnonzero(new)
    group = np.cumsum(new) - 1
    peak_db = rec["peak_db"][at]
    best = np.lexsort((band, e_pk, -peak_db.astype(np.float64), group))      # the first of every group is its peak member
    best = best[np.flatnonzero(np.concatenate(([True], group[best][1:] != group[best][:-1])))]
    out = np.zeros(len(start), dtype=EMISSION_DTYPE)
    out["row"], out["bin_lo"], out["bin_hi"] = npass[start], e_lo[start], np.maximum.reduceat(e_hi, start)
    out["peak_bin"], out["peak_db"], out["floor_db"] = e_pk[best], peak_db[best], rec["floor_db"][at][best]
    width = out["bin_hi"].astype(np.int64) - out["bin_lo"] + 1
    out["ndet"] = np.minimum(np.add.reduceat(rec["ndet"][at].astype(np.int64), start), width)
    members = np.diff(np.concatenate((start, [len(at)]))).astype(np.int32)
    return out, members, counters


def _iq_format(a):
    """FMT_* of a host array of capture blocks by its dtype: uint8, int8 and int16 are I,Q pairs, anything else is cast to
    complex64."""
    if a.dtype == np.uint8:
        return FMT_U8
    if a.dtype.kind == "i" and a.dtype.itemsize == 1:
        return FMT_S8
    if a.dtype.kind == "i" and a.dtype.itemsize == 2:
        return FMT_S16
    return FMT_C64


class ScanSurvey:
    """The survey over one engine's scan: per pass the spectra of every band, the stitch (the engine's scan state is exactly
    what scan_pass leaves), the CFAR detector over the band rows, and the stitched emission list of the pass.  It keeps the
    first `capacity` stitched records of the run and counts all of them; the detector's list is read and cleared every pass, so
    its capacity is per pass (band_capacity, sized so that a pass fits).  With `cells` it counts, per cell of total / cells elements, the passes in which a stitched
    record touched the cell.  `stream`: the stream the pass is enqueued on, set on the engine and on the detector (None: the
    default stream both start on).  The engine stays the caller's: close() leaves it open."""

    def __init__(self, engine, nsteps, train, guard, threshold_db, mode="ca", min_width=1, max_gap=0, capacity=4096, edge=0,
                 dc=0, cells=None, stream=None):
        self._det = self._trk = self._rows = self._iq = None
        n, total, hop = int(engine.fft_size), int(engine.scan_total), int(engine.scan_hop)
        if not total or not hop:
            raise KsaError("the survey needs an engine with scan geometry (scan_total_entries > 0)")
        if not _detect.MIN_NBINS <= n <= _detect.MAX_NBINS:
            raise KsaError("the survey detects band by band: fft_size %d is outside the detector's %d..%d"
                           % (n, _detect.MIN_NBINS, _detect.MAX_NBINS))
        for name, value in (("edge", edge), ("dc", dc)):
            if not 0 <= int(value) <= n // 2 - 1:
                raise KsaError("%s %d is outside 0..%d (fft_size / 2 - 1)" % (name, int(value), n // 2 - 1))
        steps = -(-total // hop)
        if int(nsteps) != steps or steps > engine.max_frames:
            raise KsaError("nsteps %d is not the engine's pass length: %d entries at a hop of %d are %d bands (max_frames %d)"
                           % (int(nsteps), total, hop, steps, engine.max_frames))
        if cells is not None and (int(cells) < 1 or total % int(cells)):
            raise KsaError("cells %d does not divide the stitched range of %d entries" % (int(cells), total))
        if not 1 <= int(capacity) <= _detect.MAX_CAPACITY:
            raise KsaError("capacity %d is outside 1..%d" % (int(capacity), _detect.MAX_CAPACITY))
        import torch                                 # plumbing only: the row buffer and the upload of host blocks
        self._torch = torch
        self.engine, self.nsteps, self.fft_size, self.total, self.hop = engine, steps, n, total, hop
        self.edge, self.dc, self.capacity, self.device = int(edge), int(dc), int(capacity), int(engine.device)
        self.cells = None if cells is None else int(cells)
        self._stream = stream
        # the detector's list is per pass: a row of n bins holds at most (n + 1) / 2 emissions, so a pass always fits (up to
        # the library's own limit), whatever `capacity` the run's list has
        self.band_capacity = min(_detect.MAX_CAPACITY, steps * ((n + 1) // 2))
        self._det = SignalDetector(n, train, guard, threshold_db, mode=mode, min_width=min_width, max_gap=max_gap,
                                   capacity=self.band_capacity, device=self.device, stream=stream)
        if stream is not None:
            engine.set_stream(stream)
        self._rows = torch.empty((steps, n), dtype=torch.float32, device="cuda:%d" % self.device)
        self._parts, self._member_parts, self._stored = [], [], 0
        self._total = 0
        self._occupancy = None if self.cells is None else np.zeros(self.cells, dtype=np.int64)
        self.passes = 0
        self.counters = dict.fromkeys(COUNTERS, 0)
        self.band_lost = 0                           # band records of passes that overran the detector's per-pass capacity

    # -- lifetime ---------------------------------------------------------------------------------
    def close(self):
        for name in ("_det", "_trk"):
            obj = getattr(self, name, None)
            if obj is not None:
                obj.close()
            setattr(self, name, None)
        self._rows = self._iq = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _open(self):
        if self._det is None:
            raise KsaError("the survey is closed")

    # -- a pass -----------------------------------------------------------------------------------
    def scan_pass(self, blocks, step_ok=None):
        """One pass from host memory: [nsteps][fullSize] complex64, or [nsteps][2 * fullSize] uint8, int8 or int16 I,Q.  The
        blocks are uploaded once; returns the stitched records of the pass."""
        self._open()
        torch = self._torch
        a = np.asarray(blocks)
        fmt = _iq_format(a)
        per = self.engine.full_size * (1 if fmt == FMT_C64 else 2)
        if fmt == FMT_C64:
            a = np.ascontiguousarray(a, dtype=np.complex64)
        else:
            a = np.ascontiguousarray(a, dtype=a.dtype.newbyteorder("="))
        if a.shape != (self.nsteps, per):
            raise KsaError("scan_pass wants [%d][%d] %s, got %s" % (self.nsteps, per, a.dtype, a.shape))
        flat = torch.from_numpy(a.view(np.float32) if fmt == FMT_C64 else a)
        if self._iq is None or self._iq.dtype != flat.dtype or self._iq.shape != flat.shape:
            self._iq = torch.empty(flat.shape, dtype=flat.dtype, device=self._rows.device)
        self._iq.copy_(flat)
        torch.cuda.current_stream(self._rows.device).synchronize()     # the copy ran on torch's stream, the pass runs on ours
        return self.scan_pass_dev(self._iq, fmt, step_ok)

    def scan_pass_dev(self, iq, fmt, step_ok=None, frame_stride=None):
        """One pass from blocks in device memory, on the one stream: spectra into the row buffer, the stitch, the detector over
        the rows, this pass's band records read and cleared, then stitch_emissions.  Returns the stitched records of the pass."""
        self._open()
        eng, det, rows = self.engine, self._det, self._rows
        if step_ok is not None and np.size(step_ok) != self.nsteps:
            raise KsaError("step_ok has %d entries for %d steps" % (np.size(step_ok), self.nsteps))
        eng.scan_spectra_dev(iq, fmt, self.nsteps, rows, step_ok, frame_stride)
        eng.scan_stitch_dev(rows, self.nsteps)
        det.detect_rows_dev(rows, self.nsteps)
        band, band_total = det.emissions()           # synchronises
        det.clear_emissions()
        self.band_lost += band_total - len(band)
        out, members, counters = stitch_emissions(band, self.nsteps, self.hop, self.fft_size, self.total, self.edge, self.dc)
        for k in COUNTERS:
            self.counters[k] += counters[k]
        room = self.capacity - self._stored
        if room > 0 and len(out):
            self._parts.append(out[:room].copy())
            self._member_parts.append(members[:room].copy())
            self._stored += len(self._parts[-1])
        self._total += len(out)
        if self._occupancy is not None and len(out):
            g = self.total // self.cells
            edges = np.zeros(self.cells + 1, dtype=np.int64)
            np.add.at(edges, out["bin_lo"] // g, 1)
            np.add.at(edges, out["bin_hi"] // g + 1, -1)
            self._occupancy += np.cumsum(edges[:-1]) > 0
        self.passes += 1
        return out

    # -- results ----------------------------------------------------------------------------------
    def emissions(self):
        """(the first `capacity` stitched records of the run in ascending (row, bin_lo) order, their members, the total)."""
        if not self._parts:
            return np.zeros(0, dtype=EMISSION_DTYPE), np.zeros(0, dtype=np.int32), self._total
        return np.concatenate(self._parts), np.concatenate(self._member_parts), self._total

    def occupancy(self):
        """int64 [cells]: the passes in which a stitched record touched the cell; None without cells."""
        return None if self._occupancy is None else self._occupancy.copy()

    def band_rows(self):
        """The device buffer float32 [nsteps][fft_size]: the band rows of the last pass."""
        self._open()
        return self._rows

    def link(self, row_gap, bin_slop, min_rows=1, min_spans=1, capacity=4096):
        """The stored records linked over the passes by an EmissionTracker over the stitched range (rows are passes, bins
        elements): (tracks, tracks_total, components_total, labels of the stored records)."""
        self._open()
        if self.total > _track.MAX_NBINS:
            raise KsaError("the stitched range of %d entries exceeds the linker's %d bins" % (self.total, _track.MAX_NBINS))
        records = self.emissions()[0]
        if self._trk is not None and self._trk.capacity != int(capacity):
            self._trk.close()
            self._trk = None
        if self._trk is None:
            self._trk = EmissionTracker(self.total, row_gap=row_gap, bin_slop=bin_slop, min_rows=min_rows, min_spans=min_spans,
                                        capacity=capacity, max_spans=self.capacity, device=self.device, stream=self._stream)
        else:
            self._trk.set_params(row_gap, bin_slop, min_rows, min_spans)
        labels = self._trk.link(records, row_end=self.passes)
        tracks, total, components = self._trk.tracks()
        return tracks, total, components, labels
