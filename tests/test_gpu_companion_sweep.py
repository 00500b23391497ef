"""The companion libraries on the GPU at the edges of their launch plans and on seeded random shapes, against their models
(tests/*_model.py) -- the cases, the plan mirrors and the guarded buffers come from tests/companion_sweep.py, which
tests/test_companion_sweep_host.py proves on the CPU (there the models' own float32 emulations are also held to the bounds at
every edge shape, with the inputs used here).

- test_plan_edges: both sides of every threshold of the five plan_for rules, and the corners of the headers.  kernel_info() of
  both objects equals the mirror (the threshold was crossed on the device); exact inputs equal the integer models' values exactly and
  float inputs stay inside the models' bounds.  Every stream is a first call that fills the history (so that every tap meets
  data and the whole LDS span holds samples) and a second of t-1, t, t+1 or 2t+3 outputs for t = the plan's tile; it then runs
  cut (a lead that fills the history, a run of pieces shorter than it, a piece of 0, of 1), bit for bit alike.
- test_random_shapes: draw(lib, COUNT, SEED) for all eleven libraries; stream form whole and cut, block form at the drawn
  strides, the list libraries' records, tables and totals exactly.
- test_every_plan_was_run: the plans seen through kernel_info() are all the mirrors enumerate.

Every device buffer is a companion_sweep.Guarded: nothing outside the ranges a call owns is written, no input is modified.

soak runs: KSA_RANDOM_CASES=200 KSA_RANDOM_SEED=7 python -m pytest tests/test_gpu_companion_sweep.py -m gpu -q"""
import importlib
import os
import time

import numpy as np
import pytest

import companion_sweep as cs
from companion_sweep import Guarded
from conftest import load_pkg

pytestmark = pytest.mark.gpu

COUNT = int(os.environ.get("KSA_RANDOM_CASES", "16"))
SEED = int(os.environ.get("KSA_RANDOM_SEED", "20201226"))
REPORT = os.environ.get("KSA_SWEEP_REPORT")      # a file that gets the lines of profiles/companion_sweep.txt
SEEN = set()                                     # (library, plan key) of every object made in this file
WORST = {}                                       # library -> worst float error / bound
T0 = time.time()


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def module_of(lib):
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd." + lib)


def report(line):
    print(line)
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(line + "\n")


# ------------------------------------------------------------------------------------------ the plan libraries
def make(A, c, ctx, max_in):
    """The object of a case, its kernel_info() held to the mirror."""
    obj = A.create(module_of(A.module), c, ctx, max_in)
    info, mirror = obj.kernel_info(), cs.plan_of(A.lib, c["shape"], c.get("type", 0))
    assert {k: info[k] for k in mirror} == mirror, (A.lib, c["shape"], info, mirror)
    assert info["grid"] >= 1 and info["vgprs"] > 0
    SEEN.add((A.lib, cs.plan_key(A.lib, mirror, c.get("type", 0))))
    return obj, info


def stream(torch, A, obj, c, src, pieces, what):
    """The pieces, one call each, from the guarded input into fresh guarded outputs whose rows lie three values further apart
    than the stream is long; returns the dense outputs [rows][total] and whatever the library lists besides (corr: events)."""
    shapes, size_in = A.outs(c), A.in_bytes(c)
    total = A.out_count(c, 0, sum(pieces))
    stride = total + 3
    outs = [Guarded.output(torch, rows * stride * size, (c.get("out_offset", 0) * size) % 16, name="%s output %d" % (what, k))
            for k, (size, rows) in enumerate(shapes)]
    seen = done = 0
    for p in pieces:
        cnt = A.out_count(c, seen, p)
        assert obj.out_count(p) == cnt, (what, seen, p)
        got = A.call(obj, c, src.ptr + seen * size_in, p, [g.ptr + done * size for g, (size, _) in zip(outs, shapes)], cnt, stride)
        assert got == cnt, (what, seen, p, got, cnt)
        for g, (size, rows) in zip(outs, shapes):
            for r in range(rows):
                g.own((r * stride + done) * size, cnt * size)
        seen, done = seen + p, done + cnt
    assert done == total
    listed = None
    if A.lib == "corr":
        obj.flush()
        listed = obj.events()
    obj.synchronize()
    for g in outs:
        g.check()
    src.check()
    return [g.read(dt).reshape(rows, stride)[:, :total].copy() for g, dt, (_, rows) in zip(outs, A.dtypes(c), shapes)], listed


def same_bits(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def streams(torch, A, c, lengths, exact, seed, cuts_for):
    """One object; for every (prefix, n) of lengths the stream of prefix + n samples, once as a call of the prefix (if any: it
    fills the history) and a call of the n samples, once cut as cuts_for says; the two compared with each other bit for bit
    and the first with the model (exact: the same values, else inside the bound).  Returns the worst error / bound (0 for
    exact inputs) and kernel_info()."""
    lengths = [(0, v) if isinstance(v, int) else v for v in lengths]
    longest = max(p + n for p, n in lengths)
    raw, ctx = cs.prepare(A, c, longest, exact, seed)
    obj, info = make(A, c, ctx, longest + 8)
    src = Guarded.input(torch, raw, (c.get("offset", 0) * A.in_bytes(c)) % 16, name="%s input" % A.lib)
    worst = 0.0
    for prefix, n in lengths:
        what = "%s %s n %d + %d %s" % (A.lib, c["shape"], prefix, n, "exact" if exact else "float")
        obj.reset()
        whole, listed = stream(torch, A, obj, c, src, [prefix, n] if prefix else [n], what + " whole")
        n += prefix
        if exact:
            A.exact_check(c, ctx, n, whole, what)
            if A.lib == "corr":
                want, total = A.exact_events(c, ctx, n)
                assert listed[1] == total and A.events_equal(listed[0], want), (what, "events", listed[1], total)
        else:
            ratio = A.float_ratio(c, ctx, n, whole)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (what, ratio)
        obj.reset()
        parts, listed2 = stream(torch, A, obj, c, src, cuts_for(n), what + " cut")
        assert same_bits(parts, whole), (what, "cut", cuts_for(n))
        if A.lib == "corr":
            assert listed2[1] == listed[1] and A.events_equal(listed2[0], listed[0]), (what, "events of the cut stream")
    obj.close()
    WORST[A.lib] = max(WORST.get(A.lib, 0.0), worst)
    return worst, info


def blocks(torch, A, c, seed):
    """The block form of a drawn case on exact inputs: rows out_pad values further apart than a block's outputs."""
    b = c["block"]
    nblocks, bl, bs, J = b["nblocks"], b["block_len"], b["block_stride"], b["J"]
    n = bs * (nblocks - 1) + bl
    raw, ctx = cs.prepare(A, c, n, True, seed)
    obj, _ = make(A, c, ctx, max(n, nblocks * bl) + 8)
    src = Guarded.input(torch, raw, (c.get("offset", 0) * A.in_bytes(c)) % 16, name="%s block input" % A.lib)
    shapes, stride = A.outs(c), J + b["out_pad"]
    outs = [Guarded.output(torch, nblocks * rows * stride * size, (c.get("out_offset", 0) * size) % 16, name="%s block output %d" % (A.lib, k))
            for k, (size, rows) in enumerate(shapes)]
    got = A.call_blocks(obj, c, src.ptr, nblocks, bl, bs, [g.ptr for g in outs], stride)
    assert got == J == A.block_count(c, bl), (A.lib, c["shape"], b, got)
    listed = obj.events() if A.lib == "corr" else None
    obj.synchronize()
    for g, (size, rows) in zip(outs, shapes):
        for r in range(nblocks * rows):
            g.own(r * stride * size, J * size)
        g.check()
    src.check()
    arrays = [g.read(dt).reshape(nblocks * rows, stride)[:, :J].copy() for g, dt, (_, rows) in zip(outs, A.dtypes(c), shapes)]
    starts = [k * bs for k in range(nblocks)]
    A.exact_blocks_check(c, ctx, starts, bl, arrays, "%s %s blocks %s" % (A.lib, c["shape"], b))
    if A.lib == "corr":
        want, total = A.exact_block_events(c, ctx, starts, bl)
        assert listed[1] == total and A.events_equal(listed[0], want), (c["shape"], b, "block events", listed[1], total)
    obj.close()


def edge_variants(e):
    """The choices an edge runs with: complex64 (demod: FM into float32) at every edge, the narrow formats, every mode and both
    output types where the edge is marked narrow."""
    if e.lib in ("ddc", "chan", "corr"):
        out = [dict(fmt=f) for f in (cs.FMTS if e.narrow else cs.FMTS[:1])]
    elif e.lib == "demod":
        out = [dict(mode=m, out=o) for m, o in ([(1, 0), (0, 0), (2, 0), (0, 1), (1, 1), (2, 1)] if e.narrow else [(1, 0)])]
    else:
        out = [dict(type=e.type, out=o) for o in ((0, 1) if e.narrow and e.type == 0 else (0,))]
    if e.lib == "corr":
        out = [dict(v, G=5, capacity=4096) for v in out]
    return out


EDGES = [e for lib in cs.PLAN_LIBS for e in cs.edge_pairs(lib)]


@pytest.mark.parametrize("edge", EDGES, ids=lambda e: "%s-%s" % (e.lib, e.name))
def test_plan_edges(torch_cuda, edge):
    A = cs.ADAPTERS[edge.lib]
    infos, worst = [], 0.0
    for side, shape in enumerate(s for s in (edge.last, edge.first) if s is not None):
        t = cs.tile_of(cs.plan_of(edge.lib, shape, edge.type))
        floated = []
        for k, variant in enumerate(edge_variants(edge)):
            c = dict(variant, lib=edge.lib, shape=shape, offset=1, out_offset=1, quarter=(side + k) % 4)
            lengths = cs.edge_streams(A, c, t)                   # the history filled first, then t-1, t, t+1, 2t+3 outputs
            seed = cs.edge_seed(edge.lib, shape, k)

            def cuts_for(n):
                return cs.edge_cuts(A, c, k, n)
            _, info = streams(torch_cuda, A, c, lengths, True, seed, cuts_for)
            fc = A.float_case(c)
            if fc not in floated:                                # the float form of a variant may be another variant's
                floated.append(fc)
                worst = max(worst, streams(torch_cuda, A, fc, lengths, False, seed + [1], cuts_for)[0])
        infos.append(info)
    if edge.first is not None:                                   # the threshold was crossed on the device
        field = ("tile_cols", "threads") if edge.field == "plan" else (edge.field,)
        assert any(infos[0][f] != infos[1][f] for f in field), (edge, infos)
    keep = ("threads", "lds_bytes", "tile_out", "tile_cols", "form")
    report("edge %s %s: %s%s; worst float error / bound %.4f" % (
        edge.lib, edge.name, " -> ".join("%s %s" % (s, {k: i[k] for k in keep if k in i}) for s, i in zip((edge.last, edge.first), infos)),
        " (type %d)" % edge.type if edge.lib == "resamp" else "", worst))


# ------------------------------------------------------------------------------------------ the random cases
def run_plan_case(torch, c):
    A = cs.ADAPTERS[c["lib"]]
    streams(torch, A, c, [c["n"]], True, c["seed"], lambda n: c["cuts"])
    streams(torch, A, A.float_case(c), [c["n"]], False, c["seed"] + 1, lambda n: c["cuts"])
    blocks(torch, A, c, c["seed"] + 2)


CASES = [c for lib in cs.LIBS for c in cs.draw(lib, COUNT, SEED)]


@pytest.mark.parametrize("case", CASES, ids=cs.case_id)
def test_random_shapes(torch_cuda, case):
    if case["lib"] in cs.PLAN_LIBS:
        run_plan_case(torch_cuda, case)
    else:
        LIST_RUNNERS[case["lib"]](torch_cuda, case)


# ------------------------------------------------------------------------------------------ the list libraries
def row_calls(torch, c, rows):
    """[(guarded input of a call's rows at the case's stride and base offset, the rows, their count)]: one per call."""
    out, at = [], 0
    for k in c["rows"]:
        part = rows[at:at + k]
        flat = cs.strided_rows(part, c["row_stride"], 0)[:(k - 1) * c["row_stride"] + c["nbins"]]
        out.append((Guarded.input(torch, flat, 4 * c["base"], name="%s rows %d.." % (c["lib"], at)), part, k))
        at += k
    return out


def run_density(torch, c):
    import density_model as dm
    rows, _ = cs.rows_input(c)
    obj = module_of("density").SpectrumDensity(c["nbins"], c["width"], c["levels"], c["lo_db"], c["hi_db"])
    want, seen = np.zeros((c["levels"] + 1, c["width"]), dtype=np.int64), 0
    calls = row_calls(torch, c, rows)
    for j, (src, part, k) in enumerate(calls):
        obj.add_rows_dev(src.ptr, k, row_stride=c["row_stride"])
        seen += dm.add_rows(want, part, c["levels"], c["lo_db"], c["hi_db"])
        if c["decay"] and j == 0:
            obj.decay(*c["decay"])
            want = dm.decay(want, *c["decay"])
    got, rows_seen = obj.read()
    assert rows_seen == seen == sum(c["rows"]) and got.dtype == want.dtype and np.array_equal(got, want), c
    assert int(got.sum()) == seen * c["nbins"] or c["decay"]
    for src, _, _ in calls:
        src.check()
    obj.close()


def run_mask(torch, c):
    import mask_model as mm
    rows, lines = cs.rows_input(c)
    obj = module_of("mask").SpectrumMask(c["nbins"], lines["upper"], lines["lower"], min_bins=c["min_bins"], capacity=c["capacity"])
    obj.set_row_base(c["row_base"])
    calls, flags = row_calls(torch, c, rows), []
    for src, part, k in calls:
        flag = Guarded.output(torch, k, c["base"], name="mask row_event").own(0, k)
        obj.check_rows_dev(src.ptr, k, row_stride=c["row_stride"], row_event=flag.ptr)
        flags.append(flag)
    want = mm.check(rows, lines["upper"], lines["lower"], c["min_bins"], c["capacity"], c["row_base"])
    hits, seen = obj.hits()
    ev, total = obj.events()
    assert seen == c["row_base"] + len(rows) and np.array_equal(hits, want["hits"]), c
    assert total == want["total"] and mm.events_equal(ev, want["events"]) and len(ev) == min(total, c["capacity"]), c
    for (src, _, _), flag in zip(calls, flags):
        src.check()
        flag.check()
    assert np.array_equal(np.concatenate([f.read(np.uint8) for f in flags]), want["event"].astype(np.uint8))
    obj.close()


def run_detect(torch, c):
    import detect_model as dm
    rows, _ = cs.rows_input(c)
    cfg = (c["train"], c["guard"], 10.0, c["mode"], c["min_width"], c["max_gap"])
    obj = module_of("detect").SignalDetector(c["nbins"], *cfg, capacity=c["capacity"])
    obj.set_row_base(c["row_base"])
    calls, outs = row_calls(torch, c, rows), []
    for src, part, k in calls:
        count = Guarded.output(torch, 4 * k, 4 * c["base"], name="detect row_count").own(0, 4 * k)
        floor = Guarded.output(torch, 4 * k * c["nbins"], 4 * c["base"], name="detect floor").own(0, 4 * k * c["nbins"])
        obj.detect_rows_dev(src.ptr, k, row_stride=c["row_stride"], row_count=count.ptr, floor=floor.ptr)
        outs.append((count, floor))
    want = dm.detect(rows, *cfg, capacity=c["capacity"], row_base=c["row_base"])
    hits, seen = obj.hits()
    ev, total = obj.emissions()
    assert seen == c["row_base"] + len(rows) and np.array_equal(hits, want["hits"]), c
    assert total == want["total"] and dm.emissions_equal(ev, want["events"]) and len(ev) == min(total, c["capacity"]), c
    for (src, _, _), (count, floor) in zip(calls, outs):
        src.check()
        count.check()
        floor.check()
    assert np.array_equal(np.concatenate([a.read(np.int32) for a, _ in outs]), want["count"])
    assert dm.floors_equal(np.concatenate([b.read(np.float32) for _, b in outs]).reshape(len(rows), c["nbins"]), want["floor"])
    obj.close()


def run_track(torch, c):
    import track_model as tm
    spans, row_end = cs.track_input(c)
    n, extra = len(spans), c["extra"] if len(spans) else 1
    junk = np.zeros(extra, dtype=tm.SPAN_DTYPE)
    junk["row"], junk["bin_lo"], junk["bin_hi"] = -5, 7, 3          # behind the count: reading one would make the list bad
    params = (c["row_gap"], c["bin_slop"], c["min_rows"], c["min_spans"])
    obj = module_of("track").EmissionTracker(c["nbins"], *params, capacity=c["capacity"], max_spans=n + extra)
    src = Guarded.input(torch, np.concatenate([spans, junk]), 8 * (c["i"] % 2), name="track spans")
    for count in (n // 2, n):                                    # every link replaces the result of the one before
        n_dev = Guarded.input(torch, np.array([count], dtype=np.int64), 8 * (c["i"] % 2), name="track count")
        labels = Guarded.output(torch, 4 * (n + extra), 4 * (c["i"] % 4), name="track labels").own(0, 4 * (n + extra))
        obj.link_dev(src.ptr, n + extra, n_dev.ptr, row_end, labels.ptr)
        rec, total, comps = obj.tracks()
        want = tm.link(spans[:count], c["nbins"], row_end, *params, capacity=c["capacity"])
        assert want[4] == 0 and total == want[1] and comps == want[2] and tm.same_records(rec, want[0]), (c, count)
        assert len(rec) == min(total, c["capacity"])
        for g in (src, n_dev, labels):
            g.check()
        got = labels.read(np.int32)
        assert np.array_equal(got[:count], want[3]) and np.all(got[count:] == -1) and np.array_equal(obj.labels(), want[3]), (c, count)
    obj.close()


def records_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and all(np.array_equal(a[k], b[k]) for k in a.dtype.names)


ON_POWER, OFF_POWER = 0.05, 0.02


def run_pulse(torch, c):
    import pulse_model as pm
    name, size = cs.FMT_NAMES[c["fmt"]], cs.SAMPLE_BYTES[c["fmt"]]
    b = c["blocks"][0]
    nb, bl, bs = b["nblocks"], b["block_len"], b["block_stride"]
    n = c["n"]
    raw = cs.bursty_raw(np.random.default_rng(c["seed"]), c["fmt"], max(n, bs * (nb - 1) + bl))
    obj = module_of("pulse").PulseDetector(c["W"], ON_POWER, OFF_POWER, c["min_len"], c["capacity"], max_in=max(n, nb * bl) + 8, fmt=name)
    src = Guarded.input(torch, raw, c["offset"] * size, name="pulse input")
    S, want, _ = pm.detect(raw[:n], c["W"], ON_POWER, OFF_POWER, c["min_len"], name)
    results = []
    for pieces in ([n], c["cuts"]):
        obj.reset()
        env = Guarded.output(torch, 8 * n, 8 * (c["i"] % 2), name="pulse env").own(0, 8 * n)
        at = 0
        for p in pieces:
            obj.process_dev(src.ptr + at * size, p, env=env.ptr + 8 * at)
            at += p
        assert obj.state()["samples_in"] == n
        obj.flush()
        ev, total, active = obj.events()
        env.check()
        src.check()
        assert np.array_equal(env.read(np.int64), S), (c, pieces[:8])
        assert total == len(want) and active == int(want["len"].sum()) and records_equal(ev, want[:c["capacity"]]), (c, pieces[:8], total, len(want))
    # the block form: every block a stream of its own from its start, flushed at its end
    obj.reset()
    stride = bl + b["out_pad"]
    env = Guarded.output(torch, 8 * nb * stride, 8 * (c["i"] % 2), name="pulse block env")
    obj.blocks_dev(src.ptr, nb, bl, block_stride=bs, env=env.ptr, out_stride=stride)
    ev, total, active = obj.events()
    parts = [pm.detect(raw[k * bs:k * bs + bl], c["W"], ON_POWER, OFF_POWER, c["min_len"], name, block=k) for k in range(nb)]
    want = np.concatenate([p[1] for p in parts])
    for k in range(nb):
        env.own(8 * k * stride, 8 * bl)
    env.check()
    src.check()
    assert np.array_equal(env.read(np.int64).reshape(nb, stride)[:, :bl], np.stack([p[0] for p in parts])), c
    assert total == len(want) and active == int(want["len"].sum()) and records_equal(ev, want[:c["capacity"]]), (c, total, len(want))
    obj.close()


def run_iqfix(torch, c):
    import iqfix_model as im
    name, size = cs.FMT_NAMES[c["fmt"]], cs.SAMPLE_BYTES[c["fmt"]]
    rng = np.random.default_rng(c["seed"])
    obj = module_of("iqfix").IqCorrector(fmt=name, max_in=max(max(b["nblocks"] * b["block_len"], b["block_stride"] * (b["nblocks"] - 1)
                                                                       + b["block_len"]) for b in c["blocks"]) + 8)
    stats, coeffs = np.zeros(6, dtype=np.int64), im.IDENTITY
    for k, b in enumerate(c["blocks"]):
        nb, bl, bs = b["nblocks"], b["block_len"], b["block_stride"]
        raw = cs.bursty_raw(rng, c["fmt"], bs * (nb - 1) + bl)
        src = Guarded.input(torch, raw, c["offset"] * size, name="iqfix input %d" % k)
        stride = bl + b["out_pad"]
        out = Guarded.output(torch, 8 * nb * stride, 8 * ((c["i"] + k) % 2), name="iqfix output %d" % k)
        obj.blocks_dev(src.ptr, nb, bl, block_stride=bs, out=out.ptr, out_stride=stride, accumulate=b["accumulate"])
        obj.synchronize()
        for j in range(nb):
            out.own(8 * j * stride, 8 * bl)
        out.check()
        src.check()
        xr, xi = im.unpack(raw, name)
        got = out.read(np.complex64).reshape(nb, stride)[:, :bl]
        for j in range(nb):
            s = slice(j * bs, j * bs + bl)
            want = im.apply(xr[s], xi[s], coeffs)
            assert np.array_equal(got[j].view(np.uint32), want.view(np.uint32)), (c, k, j)
            if b["accumulate"]:
                stats += im.stats(xr[s], xi[s])
        assert np.array_equal(obj.read_stats(), stats), (c, k)    # the totals after every call
        sol, want = obj.solve(c["mode"]), im.solve(stats, c["mode"])
        for f in ("dc_i", "dc_q", "c", "d"):
            assert np.float32(sol[f]).view(np.uint32) == np.float32(want[f]).view(np.uint32), (c, k, f, sol, want)
        assert (sol["flags"], sol["mode"], sol["count"]) == (want["flags"], want["mode"], want["count"]), (c, k, sol, want)
        coeffs = im.coeffs_of(want)
    obj.close()


LIST_RUNNERS = {"density": run_density, "mask": run_mask, "detect": run_detect, "track": run_track, "pulse": run_pulse, "iqfix": run_iqfix}


# ------------------------------------------------------------------------------------------ last: coverage and the report
def test_every_plan_was_run():
    want = {(lib, key) for lib in cs.PLAN_LIBS for key in cs.all_plans(lib)}
    assert SEEN == want, (sorted(want - SEEN), sorted(SEEN - want))
    assert all(v <= 1.0 for v in WORST.values()), WORST
    for lib in cs.PLAN_LIBS:
        report("%s: worst float error / bound %.4f; plans seen %s" % (lib, WORST.get(lib, 0.0), sorted(k for l, k in SEEN if l == lib)))
    report("%d edge cases, %d random cases (seed %d), %.1f s since the file was imported" % (len(EDGES), len(CASES), SEED, time.time() - T0))
