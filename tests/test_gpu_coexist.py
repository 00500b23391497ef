"""Objects that coexist in one process: the engine and the seven companion libraries with several live objects at once.  The
sibling files make one object, run it, compare and close it; here "correct" means that an object gives, bit for bit, what the
same object gives when it is alone, and the lone run is checked once against the library's own model (tests/*_model.py, the
oracle) by that library's bound or exactness rule.

1. a later object does not change what an earlier one may launch: the dynamic-LDS limit belongs to the kernel function, not to
   the object that set it, so every kernel function that serves more than one LDS size runs large, small, large again;
2. two objects driven in alternation, on one stream and on two, do not see each other's state;
3. four host threads, each with its own object and stream, give the sequential bits and read back their own refusal text;
4. create / close cycles give their device memory back, and closing one object leaves the others alone.

Inputs stay at or under 2^18 samples or 4096 rows.  Floats are compared as unsigned integers of their width."""
import gc
import importlib
import threading
import types

import numpy as np
import pytest

import chan_model as cm
import ddc_model as dcm
import demod_model as mm
import density_model as dnm
import detect_model as dtm
import ksa_oracle as orc
import mask_model as mkm
import resamp_model as rm
from conftest import load_pkg
from test_gpu_chan import proto
from test_gpu_ddc import INC, lowpass as ddc_lowpass, random_raw
from test_gpu_demod import lowpass as demod_lowpass
from test_gpu_density import cloud as density_cloud
from test_gpu_detect import THRESHOLD, cloud as detect_cloud
from test_gpu_mask import cloud as mask_cloud, lines_for
from test_gpu_parity import GAIN, assert_db
from test_gpu_resamp import float_input, float_taps

pytestmark = pytest.mark.gpu

MIB = 1 << 20
C64, U8, S16 = dcm.FMT_C64, dcm.FMT_U8, dcm.FMT_S16      # the engine and every companion number the formats alike
JOIN_SECONDS = 60


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def P():
    """The package and its companion modules under one name."""
    ksa = load_pkg()
    mods = {m: importlib.import_module("prgs-sdr-kspecanal_amd." + m)
            for m in ("ddc", "demod", "chan", "resamp", "density", "mask", "detect")}
    return types.SimpleNamespace(ksa=ksa, KsaError=mods["ddc"].KsaError, **mods)


def upload(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.float32) if a.dtype == np.complex64 else a).cuda()


def as_bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        return a.view(np.uint8)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64, 16: np.uint64}[a.dtype.itemsize])


def same_bits(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        ok = a.shape == b.shape and a.dtype == b.dtype and np.array_equal(as_bits(a), as_bits(b))
        assert ok, (what, k)


def cuts_of(n, pieces=5):
    """`pieces` call lengths that sum to n: none a multiple of a tile, one of them a single sample or row."""
    if pieces == 5:
        c = [n // 7 + 1, n // 3 + 2, 1, n // 5 + 3]
    else:
        c = [n // pieces + (i % 3) - 1 for i in range(pieces - 1)]
    c.append(n - sum(c))
    assert len(c) == pieces and min(c) >= 1 and sum(c) == n, (n, c)
    return c


# ------------------------------------------------------------------------------------------ the eight libraries, one shape of driver
class Lib:
    """How the tests below drive one library: make(P, shape) an object, data(shape, seed, n) for it, stage the pieces of a run
    on the device, step through them (each step one asynchronous call on the object's stream), collect outputs and final state,
    verify a lone run against the model, and provoke a refusal whose text carries the number `tag`."""
    name = ""
    room = None                                  # the capacity argument at which an object holds at least 8 MiB

    def cuts(self, n, pieces=5):
        return cuts_of(n, pieces)

    def size(self, shape, x):
        """The length of the input x in the library's unit."""
        return len(x)

    def run(self, torch, obj, shape, x, cuts):
        job = self.stage(torch, obj, shape, x, cuts)
        torch.cuda.synchronize()
        for i in range(len(cuts)):
            self.step(obj, job, i)
        return self.collect(obj, job)

    def lone(self, P, torch, shape, x, cuts, **kw):
        obj = self.make(P, shape, **kw)
        res = self.run(torch, obj, shape, x, cuts)
        obj.close()
        return res


class StreamLib(Lib):
    """ddc, demod, chan, resamp: process_dev on the next samples of one stream into a caller's buffer per call."""
    per = 2                                      # float32 (or integers) per input sample in the uploaded tensor

    def size(self, shape, x):
        return len(x) if x.dtype.kind in "cf" else len(x) // 2

    def stage(self, torch, obj, shape, x, cuts):
        dev, at = upload(torch, x), 0
        job = types.SimpleNamespace(dev=dev, ins=[], outs=[], n=list(cuts), want=[])
        for c in cuts:
            job.ins.append(dev[at * self.per:(at + c) * self.per])
            job.want.append(self.out_count(shape, at, c))
            job.outs.append(self.out_buf(torch, obj, job.want[-1]))
            at += c
        return job

    def out_buf(self, torch, obj, want):
        return torch.zeros(max(want, 1), dtype=torch.complex64, device="cuda")

    def step(self, obj, job, i):
        assert obj.process_dev(job.ins[i], job.n[i], out=job.outs[i], out_capacity=job.want[i]) == job.want[i]

    def sync(self, obj):
        obj.synchronize()

    def collect(self, obj, job):
        obj.synchronize()
        y = np.concatenate([o[:w].cpu().numpy() for o, w in zip(job.outs, job.want)])
        return {"y": y, "state": np.array(list(obj.state().values()), dtype=np.uint64)}

    def refuse(self, P, obj, job, tag):
        with pytest.raises(P.KsaError) as err:
            obj.process_dev(job.ins[0], obj.max_in + tag, out=job.outs[0], out_capacity=0)
        return str(err.value), "n_in %d exceeds max_in %d" % (obj.max_in + tag, obj.max_in)


class Ddc(StreamLib):
    name = "ddc"
    room = 1 << 22

    def make(self, P, shape, stream=None, room=None):
        fmt, D, T = shape
        return P.ddc.DownConverter(fmt, D, ddc_lowpass(P.ddc, D, T), phase_inc=INC, max_in=room or 1 << 18, stream=stream)

    def data(self, shape, seed, n):
        return random_raw(np.random.default_rng(seed), shape[0], n)

    def out_count(self, shape, at, c):
        return dcm.out_count(at, c, shape[1])

    def fn_key(self, shape, info):
        return shape[0], info["form"], info["tile_out"]

    def verify(self, P, shape, x, res):
        fmt, D, T = shape
        taps, v = ddc_lowpass(P.ddc, D, T), dcm.unpack(x, fmt)
        n = len(v)
        want = dcm.fir_at(v * dcm.rotor(dcm.phases(n, INC)), taps, D, 0, dcm.out_count(0, n, D))
        assert res["y"].shape == want.shape
        assert np.max(np.abs(res["y"].astype(np.complex128) - want)) <= dcm.bound(taps, np.abs(v).max()), shape
        assert list(res["state"]) == [n, len(want), n * INC % 2 ** 64]


class Demod(StreamLib):
    name = "demod"
    room = 1 << 23

    def make(self, P, shape, stream=None, room=None):
        mode, D, T = shape
        return P.demod.Demodulator(mode, D, demod_lowpass(P.demod, D, T), max_in=room or 1 << 18, stream=stream)

    def data(self, shape, seed, n):
        return mm.float_input(np.random.default_rng(seed), n, shape[0])

    def out_count(self, shape, at, c):
        return mm.out_count(at, c, shape[1])

    def out_buf(self, torch, obj, want):
        return torch.zeros(max(want, 1), dtype=torch.float32, device="cuda")

    def fn_key(self, shape, info):
        return shape[0], info["tile_out"]

    def verify(self, P, shape, x, res):
        mode, D, T = shape
        taps = demod_lowpass(P.demod, D, T)
        want = mm.fir_at(mm.detect(x, mode), taps, D, 0, mm.out_count(0, len(x), D))
        assert res["y"].shape == want.shape
        assert np.max(np.abs(res["y"].astype(np.float64) - want)) <= mm.bound(taps, mode, np.abs(x).max()), shape
        assert list(res["state"]) == [len(x), len(want)]


class Chan(StreamLib):
    name = "chan"
    room = 1 << 20

    def make(self, P, shape, stream=None, room=None):
        fmt, M, O, taps_per = shape
        return P.chan.Channelizer(fmt, M, O, proto(P.chan, M, taps_per), max_in=room or 1 << 18, stream=stream)

    def data(self, shape, seed, n):
        return random_raw(np.random.default_rng(seed), shape[0], n)

    def out_count(self, shape, at, c):
        return cm.out_count(at, c, shape[1] // shape[2])

    def out_buf(self, torch, obj, want):
        return torch.zeros((obj.nchan, max(want, 1)), dtype=torch.complex64, device="cuda")

    def step(self, obj, job, i):
        assert obj.process_dev(job.ins[i], job.n[i], out=job.outs[i], chan_stride=max(job.want[i], 1)) == job.want[i]

    def collect(self, obj, job):
        obj.synchronize()
        y = np.concatenate([o[:, :w].cpu().numpy() for o, w in zip(job.outs, job.want)], axis=1)
        return {"y": y, "state": np.array(list(obj.state().values()), dtype=np.uint64)}

    def refuse(self, P, obj, job, tag):
        with pytest.raises(P.KsaError) as err:
            obj.process_dev(job.ins[0], obj.max_in + tag, out=job.outs[0], chan_stride=1)
        return str(err.value), "n_in %d exceeds max_in %d" % (obj.max_in + tag, obj.max_in)

    def fn_key(self, shape, info):
        return shape[0], info["form"]

    def verify(self, P, shape, x, res):
        fmt, M, O, taps_per = shape
        assert fmt == C64
        taps = proto(P.chan, M, taps_per)
        want = cm.polyphase(x.astype(np.complex128), taps, M, O)
        assert res["y"].shape == want.shape
        assert np.max(np.abs(res["y"] - want)) <= cm.bound(taps, np.abs(x).max(), M, taps_per), shape
        assert list(res["state"])[0] == len(x)


class Resamp(StreamLib):
    name = "resamp"
    room = 1 << 21

    def taps(self, shape):
        return float_taps(np.random.default_rng(shape[1] * 1009 + shape[2] * 31 + shape[3]), shape[1:])

    def make(self, P, shape, stream=None, room=None):
        typ, L, M, taps_per = shape
        return P.resamp.Resampler(L, M, self.taps(shape), type=typ, max_in=room or 1 << 18, stream=stream)

    def data(self, shape, seed, n):
        return float_input(np.random.default_rng(seed), n, shape[0])

    def stage(self, torch, obj, shape, x, cuts):
        self.per = 2 if shape[0] == "c64" else 1
        return StreamLib.stage(self, torch, obj, shape, x, cuts)

    def out_count(self, shape, at, c):
        return rm.out_count(at, c, shape[1], shape[2])

    def out_buf(self, torch, obj, want):
        return torch.zeros(max(want, 1), dtype=torch.complex64 if obj.dtype == np.complex64 else torch.float32, device="cuda")

    def fn_key(self, shape, info):
        return shape[0], info["tile_out"]

    def verify(self, P, shape, x, res):
        typ, L, M, taps_per = shape
        taps, ms = self.taps(shape), np.arange(len(res["y"]))
        assert len(ms) == rm.cdiv(len(x) * L, M)
        want = rm.at(x.astype(np.complex128 if typ == "c64" else np.float64), taps.astype(np.float64), L, M, ms)
        assert rm.worst_ratio(res["y"], want, x, taps, L, M, ms) <= 1.0, shape
        assert list(res["state"]) == [len(x), len(ms)]


class RowLib(Lib):
    """density, mask, detect: rows of dB values accumulate in the object over several calls."""

    def stage(self, torch, obj, shape, x, cuts):
        dev, at = upload(torch, x), 0
        job = types.SimpleNamespace(dev=dev, ins=[], n=list(cuts), outs=[], host=[])
        for c in cuts:
            job.ins.append(dev[at:at + c])
            job.host.append(x[at:at + c])
            job.outs.append(self.out_buf(torch, obj, c))
            at += c
        return job

    def out_buf(self, torch, obj, nrows):
        return None

    def sync(self, obj):
        obj.synchronize()

    def refuse(self, P, obj, job, tag):
        with pytest.raises(P.KsaError) as err:
            self.rows_call(obj, job.ins[0], 1, tag)
        return str(err.value), "row_stride %d is shorter than a row of %d bins" % (tag, obj.nbins)


class Density(RowLib):
    """shape = (nbins, width, levels, path): path "dev" hands device rows over, "dev4" the same rows from a pointer 4 bytes off
    a 16-byte boundary (the 4-byte loads), "host" host rows through the staging buffer."""
    name = "density"
    LO, HI = -133.3, 7.1

    def make(self, P, shape, stream=None, room=None):
        return P.density.SpectrumDensity(shape[0], shape[1], shape[2], self.LO, self.HI, stream=stream)

    def data(self, shape, seed, n):
        return density_cloud(seed, n, shape[0], shape[2], self.LO, self.HI)

    def stage(self, torch, obj, shape, x, cuts):
        job = RowLib.stage(self, torch, obj, shape, x, cuts)
        job.path = shape[3]
        if job.path == "dev4":
            flat = torch.zeros(x.size + 4, dtype=torch.float32, device="cuda")
            flat[1:1 + x.size] = job.dev.reshape(-1)
            job.dev, at = flat, 0
            assert flat.data_ptr() % 16 == 0
            for i, c in enumerate(cuts):
                job.ins[i] = flat[1 + at * obj.nbins:]
                at += c
            assert job.ins[0].data_ptr() % 16 == 4
        return job

    def rows_call(self, obj, rows, n, stride):
        obj.add_rows_dev(rows, n, row_stride=stride)

    def step(self, obj, job, i):
        if job.path == "host":
            obj.add_rows(job.host[i])
        else:
            obj.add_rows_dev(job.ins[i], job.n[i])

    def collect(self, obj, job):
        counts, seen = obj.read()
        return {"counts": counts, "seen": np.array([seen], dtype=np.int64)}

    def fn_key(self, shape, info):
        """The add kernel's two template switches: 16-byte loads (rows of whole float4 from an aligned pointer) and shared columns."""
        return shape[0] % 4 == 0 and shape[3] != "dev4", shape[0] // shape[1] > 1

    def verify(self, P, shape, x, res):
        assert np.array_equal(res["counts"], dnm.histogram(x, shape[1], shape[2], self.LO, self.HI)) and res["seen"][0] == len(x)


class Mask(RowLib):
    """shape = (nbins, min_bins)"""
    name = "mask"
    room = 1 << 19

    def make(self, P, shape, stream=None, room=None):
        up, lo = lines_for(shape[0], True)
        return P.mask.SpectrumMask(shape[0], up, lo, min_bins=shape[1], capacity=room or 4096, stream=stream)

    def data(self, shape, seed, n):
        return mask_cloud(seed, n, shape[0], *lines_for(shape[0], True))

    def out_buf(self, torch, obj, nrows):
        return torch.full((nrows,), 7, dtype=torch.uint8, device="cuda")

    def rows_call(self, obj, rows, n, stride):
        obj.check_rows_dev(rows, n, row_stride=stride)

    def step(self, obj, job, i):
        obj.check_rows_dev(job.ins[i], job.n[i], row_event=job.outs[i])

    def collect(self, obj, job):
        hits, seen = obj.hits()
        ev, total = obj.events()
        return {"hits": hits, "seen": np.array([seen, total], dtype=np.int64), "events": ev,
                "row_event": np.concatenate([o.cpu().numpy() for o in job.outs])}

    def fn_key(self, shape, info):
        return info["vec"]

    def verify(self, P, shape, x, res):
        up, lo = lines_for(shape[0], True)
        want = mkm.check(x, up, lo, shape[1])
        assert np.array_equal(res["hits"], want["hits"]) and list(res["seen"]) == [len(x), want["total"]]
        assert mkm.events_equal(res["events"], want["events"])
        assert np.array_equal(res["row_event"], want["event"].astype(np.uint8))


class Detect(RowLib):
    """shape = (nbins, train, guard, mode, min_width, max_gap)"""
    name = "detect"
    room = 1 << 19

    def make(self, P, shape, stream=None, room=None):
        nbins, train, guard, mode, min_width, max_gap = shape
        return P.detect.SignalDetector(nbins, train, guard, THRESHOLD, mode=mode, min_width=min_width, max_gap=max_gap,
                                       capacity=room or 1 << 16, stream=stream)

    def data(self, shape, seed, n):
        return detect_cloud(seed, n, shape[0])

    def out_buf(self, torch, obj, nrows):
        return (torch.full((nrows,), -7, dtype=torch.int32, device="cuda"),
                torch.full((nrows, obj.nbins), 123.0, dtype=torch.float32, device="cuda"))

    def rows_call(self, obj, rows, n, stride):
        obj.detect_rows_dev(rows, n, row_stride=stride)

    def step(self, obj, job, i):
        obj.detect_rows_dev(job.ins[i], job.n[i], row_count=job.outs[i][0], floor=job.outs[i][1])

    def collect(self, obj, job):
        hits, seen = obj.hits()
        ev, total = obj.emissions()
        return {"hits": hits, "seen": np.array([seen, total], dtype=np.int64), "events": ev,
                "count": np.concatenate([o[0].cpu().numpy() for o in job.outs]),
                "floor": np.concatenate([o[1].cpu().numpy() for o in job.outs])}

    def fn_key(self, shape, info):
        return info["vec"]

    def verify(self, P, shape, x, res):
        nbins, train, guard, mode, min_width, max_gap = shape
        want = dtm.detect(x, train, guard, THRESHOLD, mode, min_width, max_gap, capacity=1 << 16)
        assert np.array_equal(res["hits"], want["hits"]) and list(res["seen"]) == [len(x), want["total"]]
        assert dtm.emissions_equal(res["events"], want["events"])
        assert np.array_equal(res["count"], want["count"]) and dtm.floors_equal(res["floor"], want["floor"])


class Engine(Lib):
    """shape = (fftSize, fullSize, nonOverlap, window, fmt, xRes); a unit of input is one capture block, a call one frames_dev
    batch that is committed, so that Max / Min / the running average and the waterfall ring carry from call to call."""
    name = "engine"
    room = 8192

    def cuts(self, n, pieces=5):
        c = [3, 1, 2, 5] if pieces == 5 else [1 + i % 2 for i in range(pieces - 1)]
        c.append(n - sum(c))
        assert c[-1] >= 1
        return c

    def make(self, P, shape, stream=None, room=None):
        n, full, q, window, fmt, xres = shape
        return P.ksa.SpectrumEngine(n, full_size=full, non_overlap=q, window=window, gain=GAIN, xres=xres,
                                    max_frames=room or 16, stream=stream)

    def data(self, shape, seed, n):
        full, fmt = shape[1], shape[4]
        x = (orc.synth_iq(full * n, seed) * 0.7).astype(np.complex64)
        if fmt == U8:
            return orc.quantize_u8(x).reshape(n, 2 * full)
        return x.reshape(n, full)

    def stage(self, torch, obj, shape, x, cuts):
        dev, at = upload(torch, x), 0
        job = types.SimpleNamespace(dev=dev, ins=[], n=list(cuts), outs=[], fmt=shape[4])
        for c in cuts:
            job.ins.append(dev[at:at + c])
            job.outs.append((torch.zeros((c, obj.fft_size), dtype=torch.float32, device="cuda"),
                             torch.zeros((c, obj.hm_width), dtype=torch.float32, device="cuda")))
            at += c
        return job

    def step(self, obj, job, i):
        obj.frames_dev(job.ins[i], job.fmt, job.n[i], cur_db=job.outs[i][0], hm_rows=job.outs[i][1])

    def sync(self, obj):
        obj.synchronize()

    def collect(self, obj, job):
        obj.synchronize()
        st = obj.state()
        res = {k: st[k] for k in ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg", "fftHM")}
        res["index"] = np.array([st["hm_index"], st["frames"]], dtype=np.int64)
        res["db"] = np.concatenate([o[0].cpu().numpy() for o in job.outs])
        res["rows"] = np.concatenate([o[1].cpu().numpy() for o in job.outs])
        return res

    def refuse(self, P, obj, job, tag):
        with pytest.raises(P.KsaError) as err:
            obj.frames_dev(job.ins[0], job.fmt, 1, first_index=-tag, total_frames=tag)
        return str(err.value), "batch [%d,+1) outside run of %d frames" % (-tag, tag)

    def fn_key(self, shape, info):
        return shape[4], info["path"]

    def verify(self, P, shape, x, res):
        n, full, q, window, fmt, xres = shape
        xin = orc.unpack_u8(x.reshape(-1)).reshape(len(x), full) if fmt == U8 else x
        st, db, _ = orc.zerospan_batch(xin, n, q, orc.window_table(window, n), "AVG", GAIN, xres)
        for k in ("Fft.Cur", "Fft.Max", "Fft.Min", "Fft.Avg"):
            assert_db(res[k], getattr(st, k[4:].lower()), what="%s %s" % (shape, k))
        assert_db(res["db"], db, what="%s per-frame dB" % (shape,))
        assert_db(res["rows"], np.array([orc.plotcompress(r, xres, "MAX") for r in db]), what="%s rows" % (shape,))
        assert_db(res["fftHM"], st.hm, what="%s ring" % (shape,))
        assert list(res["index"]) == [len(x) % 128, len(x)]


DDC, DEMOD, CHAN, RESAMP, DENSITY, MASK, DETECT, ENGINE = Ddc(), Demod(), Chan(), Resamp(), Density(), Mask(), Detect(), Engine()


def ddc_tile(D, T):
    """Outputs per workgroup by the down-converter's plan_for: 4, 2 or 1 per thread while 256 r outputs span at most 7680 samples,
    one per thread up to 17408, beyond that the reduce form's 8."""
    for r in (4, 2, 1):
        if (256 * r - 1) * D + T <= 7680:
            return 256 * r
    return 256 if 255 * D + T <= 17408 else 8


def units(lib, shape, tiles=3):
    """The input length of a run: a few tiles of outputs and a few more, in the library's unit (samples, rows or blocks)."""
    if lib is DDC or lib is DEMOD:
        D, T = shape[1], shape[2]
        return D * (tiles * (ddc_tile(D, T) if lib is DDC else 1024) + 7) + 1
    if lib is CHAN:
        return (shape[1] // shape[2]) * (tiles * 64 + 5) + 1
    if lib is RESAMP:
        return ((tiles * 1024 + 4) * shape[2]) // shape[1] + 1
    return min(12, (1 << 18) // shape[1]) if lib is ENGINE else 257


# ------------------------------------------------------------------------------------------ 1. a later object and the LDS limit
# (library, the large shape, the small shape, kind).  Kind "suspect": both shapes run one kernel function with different dynamic
# LDS, and the bytes are those of the library's plan_for / strip rule, worked out here by hand:
#   ddc tile form, one output per thread   (64, 1024): 64 * 271 * 8 = 138752      (16, 128): 16 * 263 * 8 = 33664
#   ddc tile form, two per thread          (14, 526): 14 * 549 * 8 = 61488        (8, 8): 8 * 513 * 8 = 32832
#   ddc tile form, four per thread         (7, 519): 7 * 1099 * 8 = 61544         (1, 1): 1024 * 8 = 8192
#   ddc reduce form, T up to four floats   (1024, 16384): 66048 + 65536 = 131584  (1024, 1): 66048 + 16 = 66064
#   density, strips of 16 columns          levels 1024: 1025 * 17 * 4 = 69700     levels 1000: 1001 * 17 * 4 = 68068
#     (only g = 1 reaches the opt-in range, so the two variants without shared columns: 16-byte loads from device rows and
#      from the staging buffer of host rows, 4-byte loads from a pointer 4 bytes off and from rows of 18 bins)
#   engine, mixed radix                    N = 15360: 122880                      N = 20: 160
# Kind "control": libraries that already keep one limit per process, or stay below the plain limit.  "one_function" asks for the
# same kernel function and different bytes, "differ" only for different bytes, "plain" for neither (the mask has no dynamic LDS).
LIMIT_CASES = [(DDC, (fmt, 64, 1024), (fmt, 16, 128), "suspect") for fmt in (C64, S16)] + \
              [(DDC, (fmt, 14, 526), (fmt, 8, 8), "suspect") for fmt in (C64, S16)] + \
              [(DDC, (fmt, 7, 519), (fmt, 1, 1), "suspect") for fmt in (C64, S16)] + \
              [(DDC, (fmt, 1024, 16384), (fmt, 1024, 1), "suspect") for fmt in (C64, S16)] + \
              [(DENSITY, (nbins, nbins, 1024, path), (nbins, nbins, 1000, path), "suspect")
               for nbins, path in ((64, "dev"), (64, "host"), (64, "dev4"), (18, "host"), (18, "dev"))] + \
              [(ENGINE, (15360, 30720, 0.5, "hanning", fmt, 512), (20, 40, 0.5, "hanning", fmt, 512), "suspect") for fmt in (C64, U8)] + \
              [(DETECT, (4096, 32, 2, "ca", 1, 0), (16, 8, 1, "ca", 1, 0), "differ"),
               (RESAMP, ("f32", 1, 16, 128), ("f32", 147, 160, 12), "differ"),          # 256 and 1024 outputs per workgroup
               (RESAMP, ("f32", 147, 160, 12), ("f32", 1, 1, 1), "one_function"),
               (MASK, (4096, 1), (64, 1), "plain")]
PLAN_BYTES = {DDC: {(64, 1024): 138752, (16, 128): 33664, (14, 526): 61488, (8, 8): 32832, (7, 519): 61544, (1, 1): 8192,
                    (1024, 16384): 131584, (1024, 1): 66064},
              DENSITY: {(64, 1024): 69700, (64, 1000): 68068, (18, 1024): 69700, (18, 1000): 68068},
              ENGINE: {(30720, 15360): 122880, (40, 20): 160}}


def limit_id(case):
    return "%s-%s-%s" % (case[0].name, "_".join(str(v) for v in case[1]), "_".join(str(v) for v in case[2]))


def guarded_run(P, torch, lib, obj, shape, x, what):
    """One whole-input run.  A launch that the runtime refuses comes back as the library's error text: the test fails with it
    and does not touch the object again, not even to free it."""
    try:
        return lib.run(torch, obj, shape, x, [lib.size(shape, x)])
    except P.KsaError as e:
        obj._h = None
        pytest.fail("%s %s, %s: refused with [%s]" % (lib.name, shape, what, e))


@pytest.mark.parametrize("order", ["large_first", "small_first"])
@pytest.mark.parametrize("case", LIMIT_CASES, ids=limit_id)
def test_a_later_object_does_not_change_what_an_earlier_one_may_launch(P, torch_cuda, case, order):
    """Large, small, large again (and small, large, small again).  The suspects set the limit per object: the down-converter to
    its plan's bytes, the density histogram to its strip's bytes in the opt-in range; the later, smaller object lowers the limit
    under the earlier one.  On ROCm 7.2.0 the runtime launches the earlier object all the same and every case passes with the
    per-object setting in place; a runtime that enforces the limit fails the suspects here, with the
    library's error text."""
    torch = torch_cuda
    lib, large, small, kind = case
    first, second = (large, small) if order == "large_first" else (small, large)
    xs = {s: lib.data(s, 1000 + i, units(lib, s)) for i, s in enumerate((large, small))}
    a = lib.make(P, first)
    ref = guarded_run(P, torch, lib, a, first, xs[first], "alone")
    lib.verify(P, first, xs[first], ref)
    b = lib.make(P, second)
    info = {first: a.kernel_info(), second: b.kernel_info()}
    if kind in ("suspect", "one_function"):
        assert lib.fn_key(large, info[large]) == lib.fn_key(small, info[small]), "the two shapes must share a kernel function"
    if kind != "plain":
        assert info[large]["lds_bytes"] > info[small]["lds_bytes"], info
    if kind == "suspect":                        # kernel_info reports the object's own bytes, over the function's static ones
        want = [PLAN_BYTES[lib][s[1:3] if lib is DDC else (s[0], s[2]) if lib is DENSITY else (s[1], s[0])] for s in (large, small)]
        assert info[large]["lds_bytes"] - info[small]["lds_bytes"] == want[0] - want[1], (info, want)
        assert 0 <= info[small]["lds_bytes"] - want[1] < 1024, (info, want)
    if lib is DENSITY:
        assert info[large]["lds_optin"] == info[small]["lds_optin"] == 1 and info[large]["strip_cols"] == info[small]["strip_cols"] == 16
    got = guarded_run(P, torch, lib, b, second, xs[second], "made second")
    lib.verify(P, second, xs[second], got)
    a.reset()
    again = guarded_run(P, torch, lib, a, first, xs[first], "again after the other object was made")
    same_bits(again, ref, (lib.name, first, "again"))
    b.reset()
    same_bits(guarded_run(P, torch, lib, b, second, xs[second], "second again"), got, (lib.name, second, "again"))
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------ 2. interleaved objects
# (library, shape of A, shape of B): the same shape twice, then two shapes that share a kernel function
PAIRS = [(DDC, (C64, 3, 11), (C64, 3, 11)), (DDC, (S16, 3, 11), (S16, 5, 35)),
         (DEMOD, (mm.MODE_FM, 3, 11), (mm.MODE_FM, 3, 11)), (DEMOD, (mm.MODE_AM, 3, 11), (mm.MODE_AM, 5, 80)),
         (CHAN, (C64, 16, 1, 4), (C64, 16, 1, 4)), (CHAN, (C64, 16, 1, 4), (C64, 64, 4, 2)),
         (RESAMP, ("c64", 2, 3, 5), ("c64", 2, 3, 5)), (RESAMP, ("f32", 2, 3, 5), ("f32", 3, 2, 8)),
         (DENSITY, (64, 64, 256, "dev"), (64, 64, 256, "dev")), (DENSITY, (64, 64, 256, "dev"), (4096, 4096, 256, "dev")),
         (MASK, (64, 1), (64, 1)), (MASK, (64, 3), (4096, 1)),
         (DETECT, (64, 8, 1, "ca", 1, 0), (64, 8, 1, "ca", 1, 0)), (DETECT, (64, 8, 1, "go", 3, 2), (1024, 32, 2, "so", 1, 70)),
         (ENGINE, (512, 1024, 0.5, "hanning", C64, 128), (512, 1024, 0.5, "hanning", C64, 128)),
         (ENGINE, (240, 960, 0.5, "hanning", U8, 60), (96, 384, 0.25, "hamming", U8, 96))]


def pair_id(pair):
    return "%s-%s-%s" % (pair[0].name, "_".join(str(v) for v in pair[1]), "_".join(str(v) for v in pair[2]))


@pytest.mark.parametrize("streams", ["one_stream", "two_streams"])
@pytest.mark.parametrize("pair", PAIRS, ids=pair_id)
def test_interleaved_objects_do_not_see_each_other(P, torch_cuda, pair, streams):
    torch = torch_cuda
    lib, shape_a, shape_b = pair
    shapes = (shape_a, shape_b)
    xs = [lib.data(s, 2000 + 17 * i, units(lib, s, tiles=2)) for i, s in enumerate(shapes)]
    cuts = [lib.cuts(lib.size(s, x)) for s, x in zip(shapes, xs)]
    assert all(len(c) >= 4 for c in cuts) and not np.array_equal(as_bits(xs[0][:4]), as_bits(xs[1][:4]))
    alone = [lib.lone(P, torch, s, x, c) for s, x, c in zip(shapes, xs, cuts)]
    for s, x, res in zip(shapes, xs, alone):
        lib.verify(P, s, x, res)
    own = [torch.cuda.Stream(), torch.cuda.Stream()] if streams == "two_streams" else [None, None]
    objs = [lib.make(P, s, stream=st.cuda_stream if st is not None else None) for s, st in zip(shapes, own)]
    if shape_a != shape_b:
        assert lib.fn_key(shape_a, objs[0].kernel_info()) == lib.fn_key(shape_b, objs[1].kernel_info()), "no shared kernel function"
    jobs = [lib.stage(torch, o, s, x, c) for o, s, x, c in zip(objs, shapes, xs, cuts)]
    torch.cuda.synchronize()
    for i in range(len(cuts[0])):                # A1 B1 A2 B2 ...: nothing synchronises in between
        for o, job in zip(objs, jobs):
            lib.step(o, job, i)
    for k, (o, job) in enumerate(zip(objs, jobs)):
        same_bits(lib.collect(o, job), alone[k], (lib.name, shapes[k], streams))
    for o in objs:
        o.close()


# ------------------------------------------------------------------------------------------ 3. host threads
THREAD_SHAPES = {ENGINE: (512, 1024, 0.5, "hanning", C64, 128), DDC: (S16, 3, 11), DEMOD: (mm.MODE_FM, 3, 11),
                 RESAMP: ("c64", 2, 3, 5)}
CALLS = 20


def threaded(P, torch, libs):
    """One thread per entry of libs, each with its own object and stream, CALLS calls each behind one barrier; half-way every
    thread provokes a refusal and reads its own text back.  Returns nothing: the results must equal the sequential runs."""
    shapes = [THREAD_SHAPES[lib] for lib in libs]
    xs = [lib.data(s, 3000 + 31 * i, 30 if lib is ENGINE else units(lib, s, tiles=2)) for i, (lib, s) in enumerate(zip(libs, shapes))]
    cuts = [lib.cuts(lib.size(s, x), CALLS) for lib, s, x in zip(libs, shapes, xs)]
    alone = [lib.lone(P, torch, s, x, c) for lib, s, x, c in zip(libs, shapes, xs, cuts)]
    for lib, s, x, res in zip(libs, shapes, xs, alone):
        lib.verify(P, s, x, res)
    own = [torch.cuda.Stream() for _ in libs]
    objs = [lib.make(P, s, stream=st.cuda_stream) for lib, s, st in zip(libs, shapes, own)]
    jobs = [lib.stage(torch, o, s, x, c) for lib, o, s, x, c in zip(libs, objs, shapes, xs, cuts)]
    torch.cuda.synchronize()
    barrier = threading.Barrier(len(libs), timeout=JOIN_SECONDS)
    texts, errors = [None] * len(libs), [None] * len(libs)

    def work(k):
        try:
            barrier.wait()
            for i in range(CALLS):
                if i == CALLS // 2:
                    texts[k] = libs[k].refuse(P, objs[k], jobs[k], 7 + k)
                libs[k].step(objs[k], jobs[k], i)
            libs[k].sync(objs[k])
        except BaseException as e:                # reported by the main thread
            errors[k] = e

    threads = [threading.Thread(target=work, args=(k,), daemon=True) for k in range(len(libs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN_SECONDS)
    assert not any(t.is_alive() for t in threads), "a thread did not come back within %d s" % JOIN_SECONDS
    assert errors == [None] * len(libs), errors
    for k, lib in enumerate(libs):
        got, want = texts[k]
        assert got == want, (lib.name, k)        # its own text, with its own number, while the others' kernels are in flight
        same_bits(lib.collect(objs[k], jobs[k]), alone[k], (lib.name, "thread", k))
    for o in objs:
        o.close()


def test_four_threads_one_library_each(P, torch_cuda):
    threaded(P, torch_cuda, [ENGINE, DDC, DEMOD, RESAMP])


@pytest.mark.parametrize("lib", [ENGINE, DDC, DEMOD, RESAMP], ids=lambda lib: lib.name)
def test_four_threads_four_objects_of_one_library(P, torch_cuda, lib):
    threaded(P, torch_cuda, [lib] * 4)


# ------------------------------------------------------------------------------------------ 4. lifetimes
LIFE_SHAPES = {ENGINE: (512, 1024, 0.5, "hanning", C64, 128), DDC: (C64, 2, 16), DEMOD: (mm.MODE_AM, 2, 16), CHAN: (C64, 16, 2, 4),
               RESAMP: ("f32", 3, 2, 8), DENSITY: (4096, 4096, 512, "dev"), MASK: (64, 1), DETECT: (64, 8, 1, "ca", 1, 0)}
LIFE_LIBS = list(LIFE_SHAPES)


def free_bytes(torch):
    """The driver's figure, after everything enqueued has finished and dropped objects were collected."""
    gc.collect()
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


@pytest.mark.parametrize("lib", LIFE_LIBS, ids=lambda lib: lib.name)
def test_sixteen_create_close_cycles_lose_less_than_one_object(P, torch_cuda, lib):
    """The free device memory lost over sixteen cycles of create, one call, close must be smaller than the footprint of one
    object, which is measured here as the drop at the warm-up's create.  The last cycle drops its object without close()."""
    torch = torch_cuda
    shape = LIFE_SHAPES[lib]
    x = lib.data(shape, 4000, units(lib, shape, tiles=1))
    probe = lib.make(P, shape, room=lib.room)
    job = lib.stage(torch, probe, shape, x, [lib.size(shape, x)])          # the caller's tensors: allocated once, outside what is measured
    probe.close()
    before = free_bytes(torch)
    obj = lib.make(P, shape, room=lib.room)
    footprint = before - free_bytes(torch)
    lib.step(obj, job, 0)
    lib.sync(obj)
    obj.close()
    print("%s: one object takes %.1f MiB of device memory" % (lib.name, footprint / MIB))
    assert footprint >= 8 * MIB, "the footprint must stand clear of the allocator's granularity"
    start = free_bytes(torch)
    for cycle in range(16):
        obj = lib.make(P, shape, room=lib.room)
        lib.step(obj, job, 0)
        lib.sync(obj)
        if cycle < 15:
            obj.close()
        del obj                                                # the last one goes through __del__
    lost = start - free_bytes(torch)
    print("%s: %d bytes lost over sixteen cycles, %d came back at the warm-up's close" % (lib.name, lost, start - (before - footprint)))
    assert lost < footprint, (lib.name, lost, footprint)
    assert start - (before - footprint) > footprint // 2, "close() must give the object's memory back promptly"


@pytest.mark.parametrize("lib", LIFE_LIBS, ids=lambda lib: lib.name)
def test_closing_one_object_leaves_the_other_alone(P, torch_cuda, lib):
    torch = torch_cuda
    shape = LIFE_SHAPES[lib] if lib is not DENSITY else (64, 64, 256, "dev")
    x = lib.data(shape, 5000, units(lib, shape, tiles=1))
    cuts = lib.cuts(lib.size(shape, x))
    alone = lib.lone(P, torch, shape, x, cuts)
    lib.verify(P, shape, x, alone)
    a, b = lib.make(P, shape), lib.make(P, shape)
    lib.run(torch, a, shape, lib.data(shape, 5001, lib.size(shape, x)), cuts)
    a.close()
    same_bits(lib.run(torch, b, shape, x, cuts), alone, (lib.name, "after the other closed"))
    a.close()                                                  # twice is harmless
    job = lib.stage(torch, b, shape, x, cuts)
    b.close()
    b.close()
    with pytest.raises(P.KsaError, match="null (argument|engine|[a-z-]+ object)"):
        lib.step(b, job, 0)
    with pytest.raises(P.KsaError, match="null (argument|engine|[a-z-]+ object)"):
        b.reset()
