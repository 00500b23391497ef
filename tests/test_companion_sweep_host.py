"""tests/companion_sweep.py proved on the CPU: the plan mirrors against the source text, the edge pairs against the mirrors, the
default seed's draws against the coverage conditions, the models' own float32 emulations against the models' bounds at every
edge and corner shape with the inputs tests/test_gpu_companion_sweep.py uses, and Guarded on CPU tensors."""
import collections
import math

import numpy as np
import pytest

import chan_model
import companion_sweep as cs
import large_model as lm
from companion_sweep import Guarded

SEED, COUNT = 20201226, 16                       # the defaults of tests/test_gpu_companion_sweep.py


# ------------------------------------------------------------------------------------------ 1. the mirrors
def test_the_mirrors_read_their_constants_from_the_source_text():
    got = lm.mirrored_constants()
    assert got == lm.EXPECTED_CONSTANTS
    assert cs.const("ddc.SPAN_SMALL") == lm.source_constant("csrc_ddc/kdc_api.hip", "SPAN_SMALL")
    assert cs.const("chan.LDS_ONE") == 2 * cs.const("chan.LDS_TWO") == lm.source_constant("csrc_chan/kch_api.hip", "LDS_ONE")
    assert cs.const("ddc.RED_WAVES") == cs.const("ddc.RED_THREADS") // 64
    assert cs.corr_lag_rule() == (2, 8, 4)
    assert cs.limit("ddc", "T") == 16384 and cs.limit("demod", "D") == 256 and cs.limit("corr", "QK") == 16384
    with pytest.raises(LookupError):
        cs.header_constant("ksa_ddc.h", "KDC_NO_SUCH_LIMIT")


def test_the_plans_the_existing_gpu_files_assert_are_the_mirrors():
    """The (tile_out, form) tests/test_gpu_ddc.py asserts, the tiles of test_gpu_demod.py and test_gpu_resamp.py and
    test_gpu_corr.py's rule: values the device has reported, so a mirror that restated a rule wrongly would show here."""
    ddc = {(1, 1): (1024, 0), (8, 64): (512, 0), (8, 3): (512, 0), (16, 128): (256, 0), (64, 1024): (256, 0), (1024, 16384): (8, 1)}
    for shape, want in ddc.items():
        assert cs.plan_key("ddc", cs.ddc_plan(*shape)) == want
    for shape, tile in {(1, 1): 1024, (5, 80): 1024, (64, 1024): 256, (256, 4096): 64}.items():
        assert cs.demod_plan(*shape)["tile_out"] == tile
    assert cs.demod_plan(64, 1024)["lds_bytes"] > 65536 > cs.demod_plan(10, 1)["lds_bytes"]
    for shape, typ, tile in [((1, 8, 16), 0, 1024), ((1, 8, 16), 1, 256), ((64, 1023, 256), 0, 256), ((1, 16, 128), 1, 256), ((147, 160, 12), 1, 1024)]:
        assert cs.resamp_plan(typ, *shape)["tile_out"] == tile
    assert cs.resamp_plan(1, 1, 16, 256)["lds_bytes"] <= 36 * 1024
    assert [cs.corr_plan(7, Q)["tile_out"] for Q in (1, 2, 3, 8)] == [2048, 2048, 1024, 1024]


def test_the_chan_mirror_is_chan_model_plan_at_every_valid_shape():
    shapes = cs.chan_shapes()
    assert len(shapes) == 808
    for s in shapes:
        p, (W, pitch, lds, threads) = cs.chan_plan(*s), chan_model.plan(*s)
        assert (p["tile_cols"], p["lds_bytes"], p["threads"]) == (W, lds, threads), s
        assert p["lds_bytes"] <= cs.const("chan.LDS_ONE") and p["threads"] >= s[0]
    count = collections.Counter(cs.plan_key("chan", cs.chan_plan(*s)) for s in shapes)
    assert len(count) == 10 and count[(32, 512)] == 80 and count[(32, 1024)] == 37 and count[(16, 1024)] == 56


def test_the_plans_stay_inside_the_lds_of_a_compute_unit():
    for lib in ("ddc", "demod"):
        for D in range(1, cs.limit(lib, "D") + 1):
            for T in cs._fir_candidates(lib, D):
                assert cs.plan_of(lib, (D, T))["lds_bytes"] <= 160 * 1024, (lib, D, T)
    assert max(cs.corr_plan(K, Q)["lds_bytes"] for K in (4096, 4095) for Q in (1, 2, 3, 4)) <= 64 * 1024


# ------------------------------------------------------------------------------------------ 2. the edges
def test_the_crossings_are_as_many_as_the_rules_give():
    ddc = collections.Counter(cs.plan_key("ddc", cs.ddc_plan(*s)) for s, _ in cs.crossings("ddc"))
    assert ddc == {(1024, 0): 7, (512, 0): 15, (256, 0): 64}
    demod = collections.Counter(cs.demod_plan(*s)["tile_out"] for s, _ in cs.crossings("demod"))
    assert demod == {1024: 4, 256: 16}
    assert [s for s, _ in cs.crossings("chan")] == [(64, 1, 31), (128, 1, 16), (128, 2, 31), (256, 1, 8), (256, 1, 16), (256, 2, 15), (256, 2, 31),
                                                    (256, 4, 19), (512, 1, 8), (512, 2, 15), (1024, 1, 4), (1024, 2, 7)]


@pytest.mark.parametrize("lib", cs.PLAN_LIBS)
def test_every_edge_pair_crosses_its_threshold(lib):
    edges = cs.edge_pairs(lib)
    pairs = [e for e in edges if e.first is not None]
    for e in edges:
        assert cs.valid(lib, e.last) and (e.first is None or cs.valid(lib, e.first)), e
    for e in pairs:
        a, b = cs.plan_of(lib, e.last, e.type), cs.plan_of(lib, e.first, e.type)
        fields = ("tile_cols", "threads") if e.field == "plan" else (e.field,)
        assert any(a[f] != b[f] for f in fields), (e, a, b)
        assert sum(x != y for x, y in zip(e.last, e.first)) == 1 and e.first[e.vary] == e.last[e.vary] + 1
        below = tuple(v - (1 if i == e.vary else 0) for i, v in enumerate(e.last))
        if cs.valid(lib, below):                                 # (at resamp's largest L the threshold lies at P = 1: nothing below)
            pb = cs.plan_of(lib, below, e.type)
            assert (pb == a) if e.field == "lds_bytes" else (cs.plan_key(lib, pb, e.type) == cs.plan_key(lib, a, e.type)), (e, "the last of its plan")
        else:
            assert lib == "resamp" and e.last[2] == 1
    shapes = {(e.last, e.type) for e in edges} | {(e.first, e.type) for e in pairs}
    want = {"ddc": {((1, 6657), 0), ((7, 520), 0), ((1, 7170), 0), ((15, 15), 0), ((5, 16134), 0), ((68, 68), 0), ((1, 16384), 0), ((1024, 1), 0)},
            "demod": {((6, 3590), 0), ((9, 522), 0), ((63, 3904), 0), ((78, 78), 0), ((255, 4096), 0), ((256, 1), 0)},
            "resamp": {((2, 19, 210), 0), ((1024, 9937, 2), 0), ((3, 14, 191), 1), ((1024, 4967, 1), 1), ((1, 16, 256), 0), ((1, 16, 256), 1)},
            "chan": {((128, 1, 17), 0), ((256, 1, 8), 0), ((256, 4, 20), 0)},
            "corr": {((64, 2), 0), ((64, 3), 0), ((4087, 1), 0), ((4088, 1), 0), ((4089, 1), 0), ((4091, 4), 0), ((4092, 4), 0), ((4093, 4), 0),
                     ((1, 8), 0), ((2048, 8), 0)}}[lib]
    assert want <= shapes, want - shapes
    assert sum(e.narrow for e in pairs) >= {"ddc": 3, "demod": 2, "resamp": 2, "chan": 3, "corr": 2}[lib]      # one pair per threshold
    if lib == "chan":
        assert len(pairs) == 12 and len(edges) == 22
        assert {cs.plan_key(lib, cs.chan_plan(*e.last)) for e in edges if e.first is None} == cs.all_plans(lib)
    assert {cs.plan_key(lib, cs.plan_of(lib, s, t), t) for s, t in shapes} == cs.all_plans(lib), "the edges alone reach every plan"


def test_all_plans_counts():
    assert {lib: len(cs.all_plans(lib)) for lib in cs.PLAN_LIBS} == {"ddc": 4, "demod": 3, "resamp": 4, "chan": 10, "corr": 2}


# ------------------------------------------------------------------------------------------ 3. the draws
@pytest.mark.parametrize("lib", cs.PLAN_LIBS)
def test_the_default_draw_of_a_plan_library_meets_the_coverage_conditions(lib):
    cases = cs.draw(lib, COUNT, SEED)
    A = cs.ADAPTERS[lib]
    assert len(cases) == COUNT and cases == cs.draw(lib, COUNT, SEED), "a draw is a function of its seed"
    assert cases != cs.draw(lib, COUNT, SEED + 1)
    for c in cases:
        assert cs.valid(lib, c["shape"]), c                      # nothing the header refuses
        assert 1 <= c["n"] <= cs.MAX_IN and sum(c["cuts"]) == c["n"] and min(c["cuts"]) >= 0
        b = c["block"]
        assert b["J"] >= 1 and b["block_len"] >= A.block_min(c) and b["nblocks"] * b["block_len"] <= cs.MAX_IN and b["block_stride"] >= 0
        assert 0 <= c["offset"] * A.in_bytes(c) < 16
        if lib == "resamp":
            L, M, P = c["shape"]
            assert math.gcd(L, M) == 1 and M <= 16 * L and not (c["type"] and c["out"])
    keys = {cs.plan_key(lib, cs.plan_of(lib, c["shape"], c.get("type", 0)), c.get("type", 0)) for c in cases}
    assert keys == cs.all_plans(lib), cs.all_plans(lib) - keys
    if lib == "chan":
        assert {(32, 512), (32, 1024), (16, 1024)} <= keys
    if lib == "corr":                                            # a capacity below the records the model produces, and one above
        totals = []
        for c in cases:
            raw, ctx = cs.prepare(A, c, c["n"], True, c["seed"])
            totals.append((A.exact_events(c, ctx, c["n"])[1], c["capacity"]))
        assert any(total > cap for total, cap in totals) and any(0 < total <= cap for total, cap in totals), totals
    if lib in ("ddc", "chan", "corr"):
        assert {c["fmt"] for c in cases} == set(cs.FMTS)
    if lib == "demod":
        assert {(c["mode"], c["out"]) for c in cases} == {(m, o) for m in (0, 1, 2) for o in (0, 1)}
    if lib == "resamp":
        assert {(c["type"], c["out"]) for c in cases} == {(0, 0), (1, 0), (0, 1)}
    assert {c["offset"] == 0 for c in cases} == {True, False} and {c["out_offset"] for c in cases} == {0, 1}
    flags = [cs.cut_flags(c["cuts"], A.hist(c)) for c in cases]
    assert any(f["zero"] for f in flags) and any(f["one"] for f in flags) and any(f["run"] for f in flags)
    strides = {(0 if c["block"]["block_stride"] == 0 else 1 if c["block"]["block_stride"] < c["block"]["block_len"] else 2) for c in cases}
    assert strides == {0, 1, 2} and {c["block"]["out_pad"] > 0 for c in cases} == {True, False}
    near = [c for c in cases if c["near"]]
    assert COUNT // 4 <= len(near) <= COUNT // 2                  # the odd cases, where the plan borders a threshold


def list_totals(c):
    """(records the model produces, the case's capacity) of a list case; (None, None) where the library lists nothing."""
    import detect_model as dm
    import mask_model as mm
    import pulse_model as pm
    import track_model as tm
    if c["lib"] == "mask":
        rows, lines = cs.rows_input(c)
        return mm.check(rows, lines["upper"], lines["lower"], c["min_bins"], c["capacity"], c["row_base"])["total"], c["capacity"]
    if c["lib"] == "detect":
        rows, _ = cs.rows_input(c)
        return dm.detect(rows, c["train"], c["guard"], 10.0, c["mode"], c["min_width"], c["max_gap"], c["capacity"], c["row_base"])["total"], c["capacity"]
    if c["lib"] == "track":
        spans, row_end = cs.track_input(c)
        got = tm.link(spans, c["nbins"], row_end, c["row_gap"], c["bin_slop"], c["min_rows"], c["min_spans"], c["capacity"])
        assert got[4] == 0 and len(spans) < c["nbins"] * c["occ_rows"] + 1, "the drawn list is a valid one"
        return got[1], c["capacity"]
    if c["lib"] == "pulse":
        raw = cs.bursty_raw(np.random.default_rng(c["seed"]), c["fmt"], c["n"])
        return len(pm.detect(raw, c["W"], 0.05, 0.02, c["min_len"], cs.FMT_NAMES[c["fmt"]])[1]), c["capacity"]
    return None, None


@pytest.mark.parametrize("lib", cs.LIST_LIBS)
def test_the_default_draw_of_a_list_library_meets_the_coverage_conditions(lib):
    cases = cs.draw(lib, COUNT, SEED)
    assert len(cases) == COUNT and cases == cs.draw(lib, COUNT, SEED) and cases != cs.draw(lib, COUNT, SEED + 1)
    if lib in ("density", "mask", "detect"):
        lo = {"density": 16, "mask": 16, "detect": 16}[lib]
        top = {"density": 1 << 20, "mask": 1 << 20, "detect": 16384}[lib]
        for c in cases:
            assert lo <= c["nbins"] <= top and sum(c["rows"]) * c["nbins"] <= cs.MAX_CELLS and min(c["rows"]) >= 1 and c["row_stride"] >= c["nbins"]
        nbins = [c["nbins"] for c in cases]
        assert lo in nbins and any(n & (n - 1) for n in nbins) and any(n > lo and not n & (n - 1) for n in nbins)
        assert {len(c["rows"]) for c in cases} == {2, 3} and {c["base"] for c in cases} == {0, 1}
        assert {c["row_stride"] > c["nbins"] for c in cases} == {True, False}
    if lib == "density":
        for c in cases:
            assert c["nbins"] % c["width"] == 0 and 1 <= c["levels"] <= 1024 and (c["levels"] + 1) * c["width"] <= 1 << 27
        assert {1, 1024} <= {c["levels"] for c in cases} and any(c["width"] == 1 for c in cases) and any(1 < c["width"] < c["nbins"] for c in cases)
        assert any(c["decay"] for c in cases)
    if lib == "mask":
        assert all(1 <= c["min_bins"] <= c["nbins"] for c in cases) and any(c["min_bins"] == c["nbins"] for c in cases)
        assert {c["lower"] for c in cases} == {True, False}
    if lib == "detect":
        for c in cases:
            assert 1 <= c["train"] <= 1024 and 0 <= c["guard"] <= 256 and 1 <= c["min_width"] <= c["nbins"] and 0 <= c["max_gap"] <= 1024
        assert {c["mode"] for c in cases} == {0, 1, 2} and any((c["train"], c["guard"]) == (1024, 256) for c in cases)
        assert any(c["max_gap"] == 1024 for c in cases)
    if lib == "track":
        for c in cases:
            assert 1 <= c["nbins"] <= 1 << 24 and c["occ_bins"] <= c["nbins"] and 0 <= c["bin_slop"] <= c["nbins"] and 0 <= c["row_gap"] <= 1024
        assert {0, 1024} <= {c["row_gap"] for c in cases} and {c["extra"] for c in cases} == {0, 7} and {1, 1 << 24} <= {c["nbins"] for c in cases}
    if lib in ("pulse", "iqfix"):
        assert {c["fmt"] for c in cases} == set(cs.FMTS) and {c["offset"] == 0 for c in cases} == {True, False}
        assert all(0 <= c["offset"] * cs.SAMPLE_BYTES[c["fmt"]] < 16 for c in cases)
        strides = {(0 if b["block_stride"] == 0 else 1 if b["block_stride"] < b["block_len"] else 2) for c in cases for b in c["blocks"]}
        assert strides == {0, 1, 2} and {b["out_pad"] > 0 for c in cases for b in c["blocks"]} == {True, False}
        assert all(b["nblocks"] * b["block_len"] <= cs.MAX_IN for c in cases for b in c["blocks"])
    if lib == "pulse":
        assert {1, 4096} <= {c["W"] for c in cases} and all(1 <= c["W"] <= 4096 and c["n"] <= cs.MAX_IN and sum(c["cuts"]) == c["n"] for c in cases)
        flags = [cs.cut_flags(c["cuts"], c["W"] - 1) for c in cases]
        assert any(f["zero"] for f in flags) and any(f["one"] for f in flags) and any(f["run"] for f in flags)
    if lib == "iqfix":
        assert {c["mode"] for c in cases} == {1, 2, 3} and {len(c["blocks"]) for c in cases} == {2, 3}
        assert any(not b["accumulate"] for c in cases for b in c["blocks"]) and all(any(b["accumulate"] for b in c["blocks"]) for c in cases)
    if lib in ("mask", "detect", "track", "pulse"):
        totals = [list_totals(c) for c in cases]
        assert any(total > cap for total, cap in totals), "a capacity below the records produced"
        assert any(0 < total <= cap for total, cap in totals)


def test_a_value_one_ulp_off_fails_the_comparisons():
    """The comparisons of the plan adapters notice one wrong bit: the exact check of a result one ulp off, the cut check's
    bytes, and a float result one bound off."""
    A = cs.ADAPTERS["ddc"]
    c = dict(lib="ddc", shape=(3, 11), fmt=cs.FMT_C64, quarter=1)
    raw, ctx = cs.prepare(A, c, 100, True, 7)
    want = A.exact_want(c, ctx, 100)
    A.exact_check(c, ctx, 100, [want[0].copy()], "clean")
    off = want[0].copy()
    off[0, 17] = np.nextafter(off[0, 17].real, np.float32(9)) + 1j * off[0, 17].imag
    with pytest.raises(AssertionError, match="first differing value"):
        A.exact_check(c, ctx, 100, [off], "one ulp")
    raw, ctx = cs.prepare(A, c, 100, False, 8)
    em = A.emulate(c, ctx, 100)
    assert A.float_ratio(c, ctx, 100, em) <= 1.0
    em[0][0, 5] += np.complex64(2.5 * A.m.bound(ctx["taps"], np.abs(ctx["x"]).max()))
    assert A.float_ratio(c, ctx, 100, em) > 1.0


def test_cuts_hold_a_run_of_pieces_shorter_than_the_history():
    rng = np.random.default_rng(5)
    for n, hist in ((1000, 10), (1000, 1), (5, 10), (0, 3), (100000, 4095), (4200, 4095), (515, 16383), (2571, 16132), (30, 2), (9, 0)):
        pieces = cs.make_cuts(rng, n, hist)
        assert sum(pieces) == n and min(pieces) >= 0 and 0 in pieces
        f = cs.cut_flags(pieces, hist)
        assert f["run"] == (hist >= 2 and n >= hist + 8), (n, hist, pieces)
        assert sum(p > 0 for p in pieces) >= (4 if n >= 6 and hist >= 2 else 2 if n >= 2 else 0), (n, hist, pieces)
    assert cs.cut_flags([10, 2, 3, 0, 1, 50], 5) == dict(zero=True, one=True, run=True)
    assert not cs.cut_flags([2, 3, 10], 5)["run"] and not cs.cut_flags([10, 2, 7, 3], 5)["run"]


# ------------------------------------------------------------------------------------------ 4. the models at the edges
def edge_cases():
    out = []
    for lib in cs.PLAN_LIBS:
        A = cs.ADAPTERS[lib]
        for shape, typ in cs.edge_shapes(lib):
            c = dict(lib=lib, shape=shape, fmt=cs.FMT_C64, mode=1, out=0, type=typ, G=5, capacity=4096, quarter=1)
            t = cs.tile_of(cs.plan_of(lib, shape, typ))
            out.append(pytest.param(A, c, sum(cs.edge_streams(A, c, t)[-1]), id="%s-%s-%d" % (lib, "x".join(map(str, shape)), typ)))
    return out


@pytest.mark.parametrize("A,c,n", edge_cases())
def test_the_float32_emulation_stays_inside_the_bound_at_every_edge_shape(A, c, n):
    """The models' own emulations (ddc_model.f32_fir behind f32_mix, demod_model.f32_fir behind f32_detect, resamp_model.f32_at,
    chan_model.f32_polyphase, corr_model.f32_chain) on the longest stream the GPU test runs at the shape, 2t + 3 outputs, with
    its inputs: the reference alone meets what the device is held to.  Every output is evaluated; no shape needed a subset."""
    seed = cs.edge_seed(A.lib, c["shape"], 0) + [1]
    raw, ctx = cs.prepare(A, c, n, False, seed)
    ratio = A.float_ratio(c, ctx, n, A.emulate(c, ctx, n))
    print("%s %s: emulation error / bound %.4f" % (A.lib, c["shape"], ratio))
    assert 0 < ratio <= 1.0, ratio


@pytest.mark.parametrize("A,c,n", edge_cases())
def test_the_exact_inputs_are_exact_in_float32_at_every_edge_shape(A, c, n):
    """The premise of the bit-for-bit comparison: on the exact inputs the float32 emulation gives the integer model's values,
    so no edge shape is exempt (chan: on the axis channels)."""
    seed = cs.edge_seed(A.lib, c["shape"], 0)
    raw, ctx = cs.prepare(A, c, n, True, seed)
    if A.lib == "ddc":
        ctx["x"] = (ctx["iq"][:, 0] + 1j * ctx["iq"][:, 1]) / ctx["scale"]
    elif A.lib == "chan":
        ctx["x"] = (ctx["iq"][:, 0] + 1j * ctx["iq"][:, 1]) / ctx["scale"]
    elif A.lib in ("demod", "resamp"):
        ctx["x"] = raw
    got = A.emulate(c, ctx, n)
    if A.lib == "corr":
        got = [got[0], (got[1] * ctx["rscale"]).astype(np.complex64)]
    A.exact_check(c, ctx, n, got, "emulation")
    if A.lib == "corr":
        ev, total = A.exact_events(c, ctx, n)
        assert total >= 1 or c["shape"][0] >= 4096 or n < 2 * c["shape"][0], "a planted copy is found"


@pytest.mark.parametrize("A,c,n", edge_cases())
def test_every_edge_stream_fills_the_history_and_is_really_cut(A, c, n):
    """Per edge shape and length: the first call brings at least the history, so that the last tap of every output of the
    second call meets a sample (and the far end of the LDS span holds data); the second call yields t-1, t, t+1, 2t+3 outputs;
    the cut has at least two pieces that are not empty, and, wherever a history exists, a piece of 0, one of 1 and a run of
    pieces shorter than the history behind a filled history."""
    t = cs.tile_of(cs.plan_of(A.lib, c["shape"], c["type"]))
    streams = cs.edge_streams(A, c, t)
    hist = A.hist(c)
    assert [A.out_count(c, p, m) for p, m in streams] == [v for v in (t - 1, t, t + 1, 2 * t + 3) if v >= 1] and sum(streams[-1]) == n
    for prefix, m in streams:
        assert prefix >= hist and m >= 1 and (m == 1 or A.out_count(c, prefix, m - 1) < A.out_count(c, prefix, m))
        first = prefix + 1 if A.lib != "corr" else prefix + m    # the sample that completes the second call's first output
        assert first - 1 - hist >= 0, "the oldest tap of the first output of the second call lies inside the stream"
        for k in range(4):
            pieces = cs.edge_cuts(A, c, k, prefix + m)
            flags = cs.cut_flags(pieces, hist)
            assert sum(pieces) == prefix + m and sum(p > 0 for p in pieces) >= 2, pieces
            assert flags["zero"] and (hist < 2 or (flags["run"] and (flags["one"] or prefix + m < hist + 8))), (hist, pieces)
    raw, ctx = cs.prepare(A, c, n, True, cs.edge_seed(A.lib, c["shape"], 0))
    taps = ctx.get("itaps", ctx.get("ftaps", ctx.get("num", ctx.get("templates"))))
    assert np.all(np.asarray(taps).reshape(-1)[[0, -1]] != 0) or A.lib == "resamp", "the outermost taps are there"
    x = np.asarray(raw).reshape(len(raw), -1) if A.lib != "chan" and A.lib != "ddc" else ctx["iq"]
    assert np.count_nonzero(np.abs(x[:max(hist, 1)]).sum(axis=-1)) >= max(hist, 1) // 4, "the history is data, not zeros"


# ------------------------------------------------------------------------------------------ 5. Guarded
def guarded_call(torch, corrupt=None):
    """A stand-in for a block call on CPU tensors: 3 rows of 5 float32 at a stride of 7 from an input of 8 complex64."""
    x = (np.arange(8) + 1j).astype(np.complex64)
    src = Guarded.input(torch, x, misalign=8, device="cpu")
    out = Guarded.output(torch, 3 * 7 * 4, misalign=4, device="cpu")
    for r in range(3):
        out.own(r * 7 * 4, 5 * 4)
        out.payload[r * 28:r * 28 + 20] = torch.from_numpy(np.full(5, r + 0.5, dtype=np.float32).view(np.uint8))
    if corrupt:
        corrupt(src, out)
    return src, out


def test_guarded_passes_a_clean_call_and_reports_every_stray_byte_with_its_offset():
    import torch
    src, out = guarded_call(torch)
    src.check()
    out.check()
    assert src.ptr % 16 == 8 and out.ptr % 16 == 4
    assert np.array_equal(out.read(np.float32).reshape(3, 7)[:, :5], np.array([[0.5] * 5, [1.5] * 5, [2.5] * 5], dtype=np.float32))
    assert np.array_equal(src.read(np.complex64), (np.arange(8) + 1j).astype(np.complex64))
    pattern = out.read(np.float32).reshape(3, 7)[:, 5:]
    assert np.all(np.isnan(pattern)) and np.all(out.read(np.int32).reshape(3, 7)[:, 5:] < 0)          # what no model produces

    def poke(g, at, value=0):
        g.buf[g.start + at] = value
    cases = [("after the owned range", lambda s, o: poke(o, 2 * 28 + 20), out, "offset 76"),
             ("before it", lambda s, o: poke(o, 28 - 1), out, "offset 27"),
             ("in a stride gap", lambda s, o: poke(o, 28 + 24), out, "offset 52"),
             ("in the guard after", lambda s, o: poke(o, 3 * 28), out, "guard after the payload was written.*offset 84"),
             ("in the guard before", lambda s, o: poke(o, -1), out, "guard before the payload was written.*offset -1"),
             ("an input byte", lambda s, o: poke(s, 13, 0x55), src, "input was modified.*offset 13"),
             ("the input's guard", lambda s, o: poke(s, 64), src, "guard after the payload was written.*offset 64")]
    for name, corrupt, _, text in cases:
        s, o = guarded_call(torch, corrupt)
        which = s if "input" in name else o
        with pytest.raises(AssertionError, match=text):
            which.check()
        (o if which is s else s).check()                         # the other buffer is still clean
    # a NaN pattern compares equal to itself (bytes, not values), and a value equal to the pattern's bytes inside an owned range is allowed
    s, o = guarded_call(torch, lambda s, o: o.payload.__setitem__(slice(0, 4), torch.tensor(list(cs.PAYLOAD_WORD), dtype=torch.uint8)))
    o.check()
    with pytest.raises(AssertionError):
        Guarded.output(torch, 16, device="cpu").own(8, 12)
