"""Launch-plan mirrors, threshold edges, seeded draws and guarded buffers for the companion libraries -- TEST INFRASTRUCTURE of
tests/test_companion_sweep_host.py (which proves all of it on the CPU) and tests/test_gpu_companion_sweep.py.

Five companions pick a launch plan from the shape in their host layer (plan_for of k??_api.hip); the kernel catalogue cannot see
that choice, so it is restated here and compared with kernel_info() on the device:

- *_plan(shape): what kernel_info() reports for the shape, from the constants of the source text (large_model.source_constant);
- edge_pairs(lib): for every threshold of the rule the last shape of one plan and the first of the next, at the smallest and the
  largest value of the other parameter at which the threshold can be met, and the corner shapes of the header;
- draw(lib, count, seed): seeded cases over the valid space, half of the shapes within +-2 of a threshold;
- Guarded: a device (or host) allocation between guard bytes, which notices any byte written outside the ranges a call owns
  and any input byte that changed.

The next companion library brings its plan mirror (if its host layer plans), its edge pairs and its draw along."""
import collections
import functools
import math
import os
import re

import numpy as np

from large_model import PKG_DIR, ROOT, mirrored_constants

PLAN_LIBS = ("ddc", "demod", "resamp", "chan", "corr")
LIST_LIBS = ("density", "mask", "detect", "track", "pulse", "iqfix")
LIBS = PLAN_LIBS + LIST_LIBS
MAX_IN = 1 << 18                                 # samples per case, as in the libraries' own GPU files
MAX_CELLS = 1 << 20                              # spectrum cells per case

FMT_C64, FMT_U8, FMT_S8, FMT_S16 = 0, 1, 2, 3
FMTS = (FMT_C64, FMT_U8, FMT_S8, FMT_S16)
FMT_NAMES = {FMT_C64: "c64", FMT_U8: "u8", FMT_S8: "s8", FMT_S16: "s16"}
SAMPLE_BYTES = {FMT_C64: 8, FMT_U8: 2, FMT_S8: 2, FMT_S16: 4}


def header_constant(header, name):
    """The integer of `#define NAME <integer>` in include/<header>; raises when the line is not there."""
    with open(os.path.join(ROOT, "include", header)) as f:
        m = re.search(r"^#define\s+%s\s+(\d+)\b" % re.escape(name), f.read(), re.M)
    if not m:
        raise LookupError("%s defines no %s" % (header, name))
    return int(m.group(1))


def corr_lag_rule():
    """(q_max, r_small, r_large) of `lags_per_thread(int Q) { return Q <= q_max ? r_small : r_large; }` in kcr_kernels.hpp."""
    with open(os.path.join(PKG_DIR, "csrc_corr/kcr_kernels.hpp")) as f:
        m = re.search(r"lags_per_thread\(int Q\)\s*\{\s*return Q <= (\d+) \? (\d+) : (\d+);", f.read())
    if not m:
        raise LookupError("kcr_kernels.hpp defines no lags_per_thread of the known form")
    return tuple(int(v) for v in m.groups())


_C = {}


def const(name):
    """A mirrored source constant ("ddc.SPAN_SMALL"), read once."""
    if not _C:
        _C.update(mirrored_constants())
    return _C[name]


LIMITS = {
    "ddc": dict(D=("ksa_ddc.h", "KDC_MAX_DECIM"), T=("ksa_ddc.h", "KDC_MAX_TAPS")),
    "demod": dict(D=("ksa_demod.h", "KDM_MAX_DECIM"), T=("ksa_demod.h", "KDM_MAX_TAPS")),
    "resamp": dict(L=("ksa_resamp.h", "KRS_MAX_L"), M=("ksa_resamp.h", "KRS_MAX_M"), ratio=("ksa_resamp.h", "KRS_MAX_RATIO"),
                   P=("ksa_resamp.h", "KRS_MAX_PHASE_TAPS"), T=("ksa_resamp.h", "KRS_MAX_TAPS")),
    "chan": dict(Mmin=("ksa_chan.h", "KCH_MIN_CHAN"), M=("ksa_chan.h", "KCH_MAX_CHAN"), P=("ksa_chan.h", "KCH_MAX_BRANCH_TAPS"),
                 T=("ksa_chan.h", "KCH_MAX_TAPS")),
    "corr": dict(K=("ksa_corr.h", "KCR_MAX_K"), Q=("ksa_corr.h", "KCR_MAX_Q"), QK=("ksa_corr.h", "KCR_MAX_TEMPLATE_VALUES")),
}
_L = {}


def limit(lib, name):
    """A limit of the library's header (limit("ddc", "T") is KDC_MAX_TAPS), read once."""
    if (lib, name) not in _L:
        _L[(lib, name)] = header_constant(*LIMITS[lib][name])
    return _L[(lib, name)]


# ------------------------------------------------------------------------------------------ the plan mirrors
def _tile_lds(tile_out, D, T, elem):
    """The tile forms of ddc and demod: D phases side by side, pitch samples each, the pitch odd where D > 1."""
    span = (tile_out - 1) * D + T
    pitch = (span + D - 1) // D
    if D > 1:
        pitch |= 1
    return D * pitch * elem


def ddc_plan(D, T):
    """kdc_api.hip plan_for: 4, 2 or 1 outputs per thread while the span stays within SPAN_SMALL, 1 up to SPAN_LARGE, else the
    reduce form."""
    threads, small, large = const("ddc.TILE_THREADS"), const("ddc.SPAN_SMALL"), const("ddc.SPAN_LARGE")
    r = next((c for c in (4, 2, 1) if (threads * c - 1) * D + T <= small), 0)
    if not r and (threads - 1) * D + T <= large:
        r = 1
    if r:
        return dict(threads=threads, tile_out=threads * r, form=0, lds_bytes=_tile_lds(threads * r, D, T, 8))
    lds = (const("ddc.RED_CHUNK") + const("ddc.RED_WAVES") * const("ddc.RED_OUT")) * 8 + ((T + 3) & ~3) * 4
    return dict(threads=const("ddc.RED_THREADS"), tile_out=const("ddc.RED_OUT"), form=1, lds_bytes=lds)


def demod_plan(D, T):
    """kdm_api.hip plan_for: 1024 outputs within SPAN_FOUR, else 256 within SPAN_TWO, else 64."""
    threads = const("demod.THREADS")                             # kdm_api.hip writes 1023, 255, 1024, 256 and 64 as literals of it
    tile = threads if (threads - 1) * D + T <= const("demod.SPAN_TWO") else threads // 4
    if (4 * threads - 1) * D + T <= const("demod.SPAN_FOUR"):
        tile = 4 * threads
    return dict(threads=const("demod.THREADS"), tile_out=tile, lds_bytes=_tile_lds(tile, D, T, 4))


def fir_thresholds(lib):
    """[(name, factor, span)] of ddc and demod: the plan changes where factor * D + T passes the span; the factors are the
    outputs of a tile less one, from the kernels' thread counts."""
    if lib == "ddc":
        t, small, large = const("ddc.TILE_THREADS"), const("ddc.SPAN_SMALL"), const("ddc.SPAN_LARGE")
        return [("four-two", 4 * t - 1, small), ("two-one", 2 * t - 1, small), ("one-reduce", t - 1, large)]
    t = const("demod.THREADS")
    return [("1024-256", 4 * t - 1, const("demod.SPAN_FOUR")), ("256-64", t - 1, const("demod.SPAN_TWO"))]


def resamp_span_bytes(W, L, M, P, elem):
    span = ((W - 1) * M + L - 1) // L + P
    return (span + (span >> 5) + 1) * elem


def resamp_plan(type, L, M, P):
    """krs_api.hip plan_for: type 0 float32, 1 complex64; 1024 outputs where their span stays within LDS_FOUR, else 256."""
    elem = 8 if type == 1 else 4
    four = 4 * const("resamp.THREADS")                           # krs_api.hip writes the 1024 as a literal
    tile = const("resamp.THREADS") * (4 if resamp_span_bytes(four, L, M, P, elem) <= const("resamp.LDS_FOUR") else 1)
    return dict(threads=const("resamp.THREADS"), tile_out=tile, lds_bytes=resamp_span_bytes(tile, L, M, P, elem))


def chan_plan(M, O, P):
    """kch_api.hip plan_for from the constants of the source; equal to chan_model.plan at every valid shape (the host test)."""
    two, one = const("chan.LDS_TWO"), const("chan.LDS_ONE")
    D, T, wmax = M // O, M * P, min(const("chan.MAX_W"), const("chan.WORK_VALUES") // M)

    def lds(W):
        return 8 * (max(M // 2, 2) + ((W * (M + 1 if W > 1 else M) + 1) & ~1) + (W - 1) * D + T)
    cands = [wmax >> s for s in range(wmax.bit_length())]
    W = next((c for c in cands if lds(c) <= two and c >= min(16, wmax)), None)
    if W is None:
        W = next(c for c in cands if lds(c) <= one)
    return dict(threads=max(M, 256 if lds(W) <= two // 2 else 512 if lds(W) <= two else 1024), tile_cols=W, form=0, lds_bytes=lds(W))


def corr_plan(K, Q):
    """kcr_api.hip plan_for: R lags per thread by lags_per_thread(Q), R rows of THREADS + ceil(K / R) + 1 complex64."""
    q_max, r_small, r_large = corr_lag_rule()
    R, threads = (r_small if Q <= q_max else r_large), const("corr.THREADS")
    return dict(threads=threads, tile_out=threads * R, lds_bytes=R * (threads + -(-K // R) + 1) * 8)


def plan_of(lib, shape, type=0):
    """The mirror of `lib` at the shape; type: resamp's element type (0 float32, 1 complex64)."""
    if lib == "resamp":
        return resamp_plan(type, *shape)
    return {"ddc": ddc_plan, "demod": demod_plan, "chan": chan_plan, "corr": corr_plan}[lib](*shape)


def plan_key(lib, plan, type=0):
    """What names a plan in the coverage sets: the fields a threshold governs, without the LDS bytes (a function of the shape)."""
    if lib == "ddc":
        return (plan["tile_out"], plan["form"])
    if lib == "chan":
        return (plan["tile_cols"], plan["threads"])
    if lib == "resamp":
        return (type, plan["tile_out"])
    return (plan["tile_out"],)


def tile_of(plan):
    return plan["tile_cols"] if "tile_cols" in plan else plan["tile_out"]


# ------------------------------------------------------------------------------------------ the valid shapes
@functools.lru_cache(maxsize=None)
def chan_shapes():
    """Every (M, O, P) kch_create accepts."""
    out, M = [], limit("chan", "Mmin")
    while M <= limit("chan", "M"):
        out += [(M, O, P) for O in (1, 2, 4) if M // O >= 1 for P in range(1, limit("chan", "P") + 1) if M * P <= limit("chan", "T")]
        M *= 2
    return tuple(out)


def resamp_valid(L, M, P):
    return (1 <= L <= limit("resamp", "L") and 1 <= M <= limit("resamp", "M") and M <= limit("resamp", "ratio") * L
            and math.gcd(L, M) == 1 and 1 <= P <= limit("resamp", "P") and L * P <= limit("resamp", "T"))


def valid(lib, shape):
    """The header's create-time rule for the shape."""
    if lib in ("ddc", "demod"):
        return 1 <= shape[0] <= limit(lib, "D") and 1 <= shape[1] <= limit(lib, "T")
    if lib == "resamp":
        return resamp_valid(*shape)
    if lib == "chan":
        return tuple(shape) in set(chan_shapes())
    K, Q = shape
    return 1 <= K <= limit("corr", "K") and 1 <= Q <= limit("corr", "Q") and K * Q <= limit("corr", "QK")


def all_plans(lib):
    """The set of plan_key the mirror gives over the library's valid shapes: what test_every_plan_was_run expects."""
    if lib == "ddc":
        return {plan_key(lib, ddc_plan(D, T)) for D in range(1, limit(lib, "D") + 1) for T in (1, limit(lib, "T"))} \
            | {plan_key(lib, ddc_plan(1, T)) for T in range(1, limit(lib, "T") + 1, 64)}
    if lib == "demod":
        return {plan_key(lib, demod_plan(D, T)) for D in range(1, limit(lib, "D") + 1) for T in (1, limit(lib, "T"))}
    if lib == "resamp":
        return {(t, resamp_plan(t, L, M, P + d)["tile_out"]) for t in (0, 1) for L, v in resamp_crossings(t).items() for M, P in v[:1] for d in (0, 1)}
    if lib == "chan":
        return {plan_key(lib, chan_plan(*s)) for s in chan_shapes()}
    return {plan_key(lib, corr_plan(1, Q)) for Q in range(1, limit("corr", "Q") + 1)}


# ------------------------------------------------------------------------------------------ the edges
# last: the last shape of its plan along `vary` (the index of the varying parameter); first: the same shape with that parameter
# one larger, the first of the next plan; field: the kernel_info field the threshold governs.  A corner or an interior shape has
# first None.  narrow: the pair at which the narrow formats, every mode and both output types also run.  type: resamp's.
Edge = collections.namedtuple("Edge", "lib name last first vary field narrow type")


def _edge(lib, name, last, vary=None, field=None, narrow=False, type=0):
    first = None
    if vary is not None:
        first = tuple(v + (1 if i == vary else 0) for i, v in enumerate(last))
    return Edge(lib, name, tuple(last), first, vary, field, narrow, type)


def _fir_edges(lib, plan, thresholds):
    """ddc and demod: thresholds = [(name, factor, span constant)]: the plan changes where factor * D + T passes the span."""
    out = []
    for name, factor, span in thresholds:
        ds = [D for D in range(1, limit(lib, "D") + 1) if 1 <= span - factor * D < limit(lib, "T")
              and plan(D, span - factor * D)["tile_out"] != plan(D, span - factor * D + 1)["tile_out"]]
        for i, D in enumerate((ds[0], ds[-1])):
            out.append(_edge(lib, "%s-D%d" % (name, D), (D, span - factor * D), 1, "tile_out", narrow=i == 0))
    return out


@functools.lru_cache(maxsize=None)
def crossings(lib, type=0):
    """Every (last shape, varying index) at which the mirror's plan changes when the varying parameter (T, P or Q) grows by one
    and both shapes are valid -- the whole list that edge_pairs picks from, and whose length the issue of this sweep counted."""
    if lib in ("ddc", "demod"):
        plan = ddc_plan if lib == "ddc" else demod_plan
        out = []
        for D in range(1, limit(lib, "D") + 1):
            out += [((D, T), 1) for T in _fir_candidates(lib, D)
                    if T < limit(lib, "T") and plan(D, T)["tile_out"] != plan(D, T + 1)["tile_out"]]
        return out
    if lib == "chan":
        ok = set(chan_shapes())
        return [((M, O, P), 2) for (M, O, P) in chan_shapes()
                if (M, O, P + 1) in ok and plan_key(lib, chan_plan(M, O, P)) != plan_key(lib, chan_plan(M, O, P + 1))]
    raise ValueError(lib)


def _fir_candidates(lib, D):
    """The T at which a plan of ddc or demod can change for this D, each with its successor: the thresholds' own T and T + 1."""
    ts = {1, limit(lib, "T")}
    for _, factor, span in fir_thresholds(lib):
        t = span - factor * D
        ts.update(v for v in (t - 1, t, t + 1, t + 2) if 1 <= v <= limit(lib, "T"))
    return sorted(ts)


@functools.lru_cache(maxsize=None)
def resamp_crossings(type):
    """{L: [(M, P)]}: for every L the (M, P) with P < KRS_MAX_PHASE_TAPS whose plan differs from (M, P + 1)'s, both valid."""
    elem, lds = (8 if type == 1 else 4), const("resamp.LDS_FOUR")
    out = {}
    for L in range(1, limit("resamp", "L") + 1):
        pmax = min(limit("resamp", "P"), limit("resamp", "T") // L)
        M = np.arange(1, min(limit("resamp", "M"), limit("resamp", "ratio") * L) + 1, dtype=np.int64)
        base = ((4 * const("resamp.THREADS") - 1) * M + L - 1) // L      # the span of a four-per-thread tile without its P
        fits = lambda P: (base + P + ((base + P) >> 5) + 1) * elem <= lds
        for m in M[fits(1) & ~fits(pmax) & (np.gcd(M, L) == 1)]:
            P = max(p for p in range(1, pmax) if resamp_span_bytes(4 * const("resamp.THREADS"), L, int(m), p, elem) <= lds)
            out.setdefault(L, []).append((int(m), P))
    return out


@functools.lru_cache(maxsize=None)
def edge_pairs(lib):
    """[Edge] of the library: two crossings per threshold and the corners (see the module's text and the Edge fields)."""
    if lib == "ddc":
        out = _fir_edges(lib, ddc_plan, fir_thresholds(lib))
        return out + [_edge(lib, "corner-T", (1, limit(lib, "T"))), _edge(lib, "corner-D", (limit(lib, "D"), 1))]
    if lib == "demod":
        out = _fir_edges(lib, demod_plan, fir_thresholds(lib))
        return out + [_edge(lib, "corner-T", (limit(lib, "D") - 1, limit(lib, "T"))), _edge(lib, "corner-D", (limit(lib, "D"), 1))]
    if lib == "resamp":
        out = []
        for type, tname in ((0, "f32"), (1, "c64")):
            cr = resamp_crossings(type)
            for i, L in enumerate((min(cr), max(cr))):
                M, P = max(cr[L])                                   # the largest M: the crossing at the fewest taps per phase
                out.append(_edge(lib, "%s-L%d" % (tname, L), (L, M, P), 2, "tile_out", narrow=i == 0, type=type))
            out.append(_edge(lib, "%s-corner-P" % tname, (1, limit(lib, "ratio"), limit(lib, "P")), type=type))
        return out
    if lib == "chan":
        out = [_edge(lib, "M%d-O%d-P%d" % s, s, 2, "plan", narrow=i % 4 == 0) for i, (s, _) in enumerate(crossings(lib))]
        seen = {}
        for s in chan_shapes():                                  # one interior shape per plan: neither side of a crossing
            key = plan_key(lib, chan_plan(*s))
            near = [chan_plan(s[0], s[1], p) for p in (s[2] - 1, s[2] + 1) if (s[0], s[1], p) in set(chan_shapes())]
            if key not in seen and all(plan_key(lib, n) == key for n in near):
                seen[key] = s
        return out + [_edge(lib, "interior-W%d-%d" % key, s) for key, s in sorted(seen.items())]
    q_max, r_small, r_large = corr_lag_rule()
    kmax, qmax = limit("corr", "K"), limit("corr", "Q")
    out = [_edge(lib, "Q%d-Q%d" % (q_max, q_max + 1), (64, q_max), 1, "tile_out", narrow=True)]
    for Q, R in ((1, r_small), (4, r_large)):
        c = (kmax - 1) // R                                      # the largest c with c R + 1 <= KCR_MAX_K
        out.append(_edge(lib, "row-Q%d" % Q, (c * R, Q), 0, "lds_bytes", narrow=Q == 1))
        out.append(_edge(lib, "row-Q%d-below" % Q, (c * R - 1, Q)))
    return out + [_edge(lib, "corner-K1", (1, qmax)), _edge(lib, "corner-QK", (limit("corr", "QK") // qmax, qmax))]


def edge_shapes(lib):
    """[(shape, type)] of every shape edge_pairs names, in order, once each."""
    out = []
    for e in edge_pairs(lib):
        for s in (e.last, e.first):
            if s is not None and (s, e.type) not in out:
                out.append((s, e.type))
    return out


# ------------------------------------------------------------------------------------------ guarded buffers
# Two byte patterns, each a 4-byte word repeated from the first byte of its region.  Read as float32 both are NaNs whose payload
# no arithmetic produces (the hardware's own NaN is 0x7fc00000, and no input holds one); the payload word is a negative int32
# and int64 (-5913691 ...: counts, bins, rows and positions are never negative, a stream's block field is -1), the guard word
# is above 2^30, beyond every count and index of these cases, and as int64 beyond 2^52, the largest position.  Every int16 is a
# value PCM output can take, so there the words hold two different halves (-15451, -91 and -11549, 32689): a run of stray
# stores cannot repeat them, a single stray store has one chance in 65536.  The two words differ in every byte, so a write
# of one region's pattern into the other shows too.
PAYLOAD_WORD = bytes((0xA5, 0xC3, 0xA5, 0xFF))
GUARD_WORD = bytes((0xE3, 0xD2, 0xB1, 0x7F))
GUARD_BYTES = 256


def _pattern(word, nbytes):
    return np.frombuffer((word * (nbytes // 4 + 1))[:nbytes], dtype=np.uint8).copy()


class Guarded:
    """A uint8 torch tensor of GUARD_BYTES guard bytes, a payload of nbytes whose address is `misalign` mod 16, and GUARD_BYTES
    more guard bytes.  An output's payload starts as PAYLOAD_WORD repeated, an input's as the uploaded bytes, of which a host
    copy is kept.  own(offset, nbytes) names a range a call may write; check() asserts that both guards still hold their pattern,
    that an input is bit-identical to what was uploaded, and that an output holds the payload pattern outside the owned ranges.
    Works on any device torch has, "cpu" included."""

    def __init__(self, torch, nbytes, misalign=0, device="cuda", name="buffer"):
        assert 0 <= misalign < 16 and nbytes >= 0
        self.torch, self.nbytes, self.name, self.owned, self.upload = torch, int(nbytes), name, [], None
        self.buf = torch.empty(2 * GUARD_BYTES + 16 + self.nbytes, dtype=torch.uint8, device=device)
        self.start = GUARD_BYTES + (misalign - (self.buf.data_ptr() + GUARD_BYTES)) % 16
        self.ptr = self.buf.data_ptr() + self.start
        assert self.ptr % 16 == misalign
        self._put(0, _pattern(GUARD_WORD, self.start))
        self._put(self.start + self.nbytes, _pattern(GUARD_WORD, len(self.buf) - self.start - self.nbytes))

    def _put(self, at, host_bytes):
        if len(host_bytes):
            self.buf[at:at + len(host_bytes)] = self.torch.from_numpy(host_bytes).to(self.buf.device)

    @classmethod
    def output(cls, torch, nbytes, misalign=0, device="cuda", name="output"):
        g = cls(torch, nbytes, misalign, device, name)
        g._put(g.start, _pattern(PAYLOAD_WORD, g.nbytes))
        return g

    @classmethod
    def input(cls, torch, array, misalign=0, device="cuda", name="input"):
        host = np.ascontiguousarray(array).view(np.uint8).reshape(-1).copy()
        g = cls(torch, len(host), misalign, device, name)
        g.upload = host
        g._put(g.start, host)
        return g

    @property
    def payload(self):
        return self.buf[self.start:self.start + self.nbytes]

    def own(self, offset, nbytes):
        """A call may write payload bytes [offset, offset + nbytes)."""
        assert 0 <= offset and offset + nbytes <= self.nbytes, (self.name, offset, nbytes, self.nbytes)
        if nbytes > 0:
            self.owned.append((int(offset), int(nbytes)))
        return self

    def read(self, dtype, count=None, offset=0):
        """numpy array of `count` values of dtype from payload byte `offset` (the whole payload by default)."""
        host = self.payload.cpu().numpy()
        size = np.dtype(dtype).itemsize
        count = (self.nbytes - offset) // size if count is None else count
        return host[offset:offset + count * size].copy().view(dtype)

    def _same(self, lo, hi, want, what):
        got = self.buf[lo:hi]
        if self.torch.equal(got.cpu(), self.torch.from_numpy(want)):
            return
        host = got.cpu().numpy()
        bad = np.flatnonzero(host != want)
        assert np.array_equal(host, want), "%s: %s, %d bytes differ, the first at payload offset %d (0x%02x, not 0x%02x)" % (
            self.name, what, len(bad), lo + int(bad[0]) - self.start, host[bad[0]], want[bad[0]])

    def check(self):
        end = self.start + self.nbytes
        self._same(0, self.start, _pattern(GUARD_WORD, self.start), "the guard before the payload was written")
        self._same(end, len(self.buf), _pattern(GUARD_WORD, len(self.buf) - end), "the guard after the payload was written")
        if self.upload is not None:
            self._same(self.start, end, self.upload, "the input was modified")
            return
        host = self.payload.cpu().numpy()
        want = _pattern(PAYLOAD_WORD, self.nbytes)
        free = np.ones(self.nbytes, dtype=bool)
        for lo, n in self.owned:
            free[lo:lo + n] = False
        bad = np.flatnonzero(free & (host != want))
        assert not len(bad), "%s: %d bytes outside the ranges the calls own were written, the first at payload offset %d (0x%02x)" % (
            self.name, len(bad), int(bad[0]), host[bad[0]])


# ------------------------------------------------------------------------------------------ cuts
def make_cuts(rng, n, hist):
    """Pieces that sum to n: a lead of at least `hist` samples (so that the history holds data) that leaves three quarters of
    what lies beyond to the rest, a run of three pieces of 1 .. hist - 1 samples each (each shorter than the history: a history
    kernel then builds its rows from the previous history) that take at most a quarter of what is left each, a piece of 0 and
    one of 1 sample, up to three random pieces, the rest.  A stream no longer than the history leads with half of itself or
    less, so that it is cut all the same.  Only what does not fit into n comes out as 0: from n = 6 on (and hist >= 2) at
    least four pieces are not empty."""
    pieces, left = [], int(n)

    def take(k):
        nonlocal left
        k = min(int(k), left)
        pieces.append(k)
        left -= k
    lead = hist if n > hist else n // 2
    take(rng.integers(lead, lead + (n - lead) // 4 + 1))
    for _ in range(3):
        top = min(hist, left // 4 + 2)                           # exclusive
        take(rng.integers(1, top) if top >= 2 else 0)
    take(0)
    take(1)
    for _ in range(int(rng.integers(1, 4))):
        take(rng.integers(0, left // 2 + 2))
    pieces.append(left)
    return pieces


def cut_flags(pieces, hist):
    """dict(zero, one, run): a piece of 0 samples, of 1 sample, and two or more consecutive pieces of 1 .. hist - 1 samples after
    at least hist samples."""
    seen, run, best = 0, 0, 0
    for p in pieces:
        run = run + 1 if (1 <= p < hist and seen >= hist) else 0
        best, seen = max(best, run), seen + p
    return dict(zero=0 in pieces, one=1 in pieces, run=best >= 2)


def _int_taps(rng, T, most):
    taps = rng.integers(-most, most + 1, T)
    taps[0], taps[-1] = most, -max(1, most - 1)                  # the outermost taps are there
    return taps


def _int_raw(rng, fmt, n, amp):
    """Raw samples whose integer values stay within +-amp (uint8: around 128; complex64: k / 2^15)."""
    b = rng.integers(-amp, amp + 1, 2 * n)
    if fmt == FMT_C64:
        return ((b[0::2] + 1j * b[1::2]) / 32768.0).astype(np.complex64)
    if fmt == FMT_U8:
        return (b + 128).astype(np.uint8)
    return b.astype(np.int8 if fmt == FMT_S8 else np.int16)


def _float_raw(rng, fmt, n):
    if fmt == FMT_C64:
        return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)
    lo, hi, dtype = {FMT_U8: (0, 256, np.uint8), FMT_S8: (-128, 128, np.int8), FMT_S16: (-32768, 32768, np.int16)}[fmt]
    return rng.integers(lo, hi, 2 * n).astype(dtype)


def _lowpass(rng, T, D):
    """float32 [T]: a windowed sinc of unit sum with a random dither, so that no two taps are equal."""
    t = np.arange(T, dtype=np.float64) - (T - 1) / 2
    h = np.sinc(0.8 * t / max(D, 1)) * np.hamming(T + 2)[1:-1] * rng.uniform(0.9, 1.1, T)
    return (h / np.abs(h).sum()).astype(np.float32)


def _fmt_amp(fmt):
    return {FMT_C64: 32767, FMT_U8: 127, FMT_S8: 127, FMT_S16: 32767}[fmt]


# ------------------------------------------------------------------------------------------ the plan libraries' adapters
# One class per library: what a case needs from the models, and the calls on the wrapper object.  A case c is a dict with
# shape and the library's own choices (fmt / mode / type / out); n is the length of a stream.  outs: [(bytes per value, rows)]
# of the dense outputs of a stream call; a call writes `cnt` values per row from value `done` on, rows `stride` values apart.
class Ddc:
    lib, module, cls = "ddc", "ddc", "DownConverter"
    import ddc_model as m

    @classmethod
    def create(cls, X, c, ctx, max_in):
        return X.DownConverter(c["fmt"], c["shape"][0], ctx["taps"], phase_inc=ctx["inc"], max_in=max_in, u8_offset=128.0, u8_scale=128.0)

    @staticmethod
    def hist(c):
        return c["shape"][1] - 1

    @staticmethod
    def in_bytes(c):
        return SAMPLE_BYTES[c["fmt"]]

    @staticmethod
    def outs(c):
        return [(8, 1)]

    @staticmethod
    def need(c, count):
        return c["shape"][0] * (count - 1) + 1

    @classmethod
    def out_count(cls, c, seen, n):
        return cls.m.out_count(seen, n, c["shape"][0])

    @classmethod
    def exact(cls, rng, c, n):
        D, T = c["shape"]
        most = 8 if T <= 64 else 1
        taps = _int_taps(rng, T, most)
        amp = max(1, min(_fmt_amp(c["fmt"]), 2 ** 23 // (T * most)))     # T max|h| max|b| <= 2^23: every partial sum is a float32
        raw = _int_raw(rng, c["fmt"], n, amp)
        iq, scale = cls.m.to_int(raw, c["fmt"])
        return raw, dict(taps=taps.astype(np.float32), itaps=taps, iq=iq, scale=scale, inc=c.get("quarter", 0) * 2 ** 62)

    @classmethod
    def exact_want(cls, c, ctx, n):
        D = c["shape"][0]
        return [cls.m.int_stream(ctx["iq"][:n], ctx["scale"], ctx["itaps"], D, cls.m.phases(n, ctx["inc"]))[None, :]]

    @classmethod
    def exact_blocks(cls, c, ctx, starts, block_len):
        D = c["shape"][0]
        return [cls.m.int_blocks(ctx["iq"], ctx["scale"], ctx["itaps"], D, ctx["inc"], len(starts), block_len, starts)]

    @staticmethod
    def block_min(c):
        return c["shape"][1]

    @staticmethod
    def block_count(c, block_len):
        return (block_len - c["shape"][1]) // c["shape"][0] + 1

    @classmethod
    def floats(cls, rng, c, n):
        D, T = c["shape"]
        raw = _float_raw(rng, c["fmt"], n)
        return raw, dict(taps=_lowpass(rng, T, D), x=cls.m.unpack(raw, c["fmt"], 128.0, 128.0), inc=int(rng.integers(1, 2 ** 63)) | 1)

    @classmethod
    def float_ratio(cls, c, ctx, n, got):
        """Worst error / ddc_model.bound of a stream result [[count]] against the float64 model."""
        D = c["shape"][0]
        if "_fwant" not in ctx:                                  # once for the whole input: a shorter stream's outputs are a prefix
            full = ctx["n"]
            ctx["_fwant"] = cls.m.fir_at(ctx["x"] * cls.m.rotor(cls.m.phases(full, ctx["inc"])), ctx["taps"], D, 0, cls.m.out_count(0, full, D))
        want = ctx["_fwant"][:cls.m.out_count(0, n, D)]
        assert got[0].shape == (1, len(want))
        limit = cls.m.bound(ctx["taps"], np.abs(ctx["x"][:n]).max(initial=0.0))
        return float(np.max(np.abs(got[0][0].astype(np.complex128) - want), initial=0.0)) / limit if limit else 0.0

    @classmethod
    def emulate(cls, c, ctx, n):
        """The model's own float32 emulation, shaped as a device result."""
        D = c["shape"][0]
        v = cls.m.f32_mix(ctx["x"][:n].astype(np.complex64), cls.m.phases(n, ctx["inc"]))
        return [cls.m.f32_fir(v, ctx["taps"], D, 0, cls.m.out_count(0, n, D))[None, :]]

    @staticmethod
    def call(obj, c, in_ptr, n, ptrs, cnt, stride):
        return obj.process_dev(in_ptr, n, out=ptrs[0], out_capacity=cnt)

    @staticmethod
    def call_blocks(obj, c, in_ptr, nblocks, block_len, block_stride, ptrs, out_stride):
        return obj.blocks_dev(in_ptr, nblocks, block_len, block_stride=block_stride, out=ptrs[0], out_stride=out_stride)

    @staticmethod
    def dtypes(c):
        return [np.complex64]

    @staticmethod
    def float_case(c):
        return c


class Demod:
    lib, module = "demod", "demod"
    import demod_model as m

    @classmethod
    def create(cls, X, c, ctx, max_in):
        return X.Demodulator(c["mode"], c["shape"][0], ctx["taps"], out_fmt="s16" if c["out"] else "f32",
                             pcm_scale=ctx.get("pcm_scale", 32767.0), max_in=max_in)

    @staticmethod
    def hist(c):
        return c["shape"][1] - 1

    @staticmethod
    def in_bytes(c):
        return 8

    @staticmethod
    def outs(c):
        return [(2 if c["out"] else 4, 1)]

    @staticmethod
    def dtypes(c):
        return [np.int16 if c["out"] else np.float32]

    @staticmethod
    def need(c, count):
        return c["shape"][0] * (count - 1) + 1

    @classmethod
    def out_count(cls, c, seen, n):
        return cls.m.out_count(seen, n, c["shape"][0])

    @classmethod
    def exact(cls, rng, c, n):
        D, T = c["shape"]
        most = 8 if T <= 64 else max(1, min(4, 2 ** 21 // (T * 123)))    # 4 T max|h| max|d| < 2^24 in quarters of the detector's unit
        taps = _int_taps(rng, T, most).astype(np.float64)
        if T >= 4:
            taps[1], taps[2] = 0.5, -0.25                          # powers of two among the small integers
        if c["mode"] == cls.m.MODE_AM:
            x, mag = cls.m.exact_am_samples(rng, n)
            dn, dden = cls.m.exact_detect(c["mode"], mag=mag)
        else:
            x, k = cls.m.exact_turn_samples(rng, n)
            dn, dden = cls.m.exact_detect(c["mode"], k=k)
        conv = cls.m.exact_conv(dn, dden, taps)
        y = np.abs(cls.m.exact_stream(dn, dden, taps, D, conv=conv).astype(np.float64))
        scale = 2.0 ** np.ceil(np.log2(32768 / np.median(y[y > 0]))) if np.any(y > 0) else 1.0     # half of the values saturate
        return x, dict(taps=taps.astype(np.float32), ftaps=taps, dn=dn, dden=dden, conv=conv, pcm_scale=float(min(max(scale, 1.0), 2.0 ** 19)))

    @classmethod
    def exact_want(cls, c, ctx, n):
        return [cls.m.exact_stream(ctx["dn"][:n], ctx["dden"], ctx["ftaps"], c["shape"][0], c["out"], ctx["pcm_scale"], conv=ctx["conv"])[None, :]]

    @classmethod
    def exact_blocks(cls, c, ctx, starts, block_len):
        return [cls.m.exact_blocks(ctx["dn"], ctx["dden"], ctx["ftaps"], c["shape"][0], c["mode"], starts, block_len, c["out"],
                                   ctx["pcm_scale"], conv=ctx["conv"])]

    @classmethod
    def block_min(cls, c):
        return cls.m.lead(c["mode"]) + c["shape"][1]

    @classmethod
    def block_count(cls, c, block_len):
        return cls.m.block_out_count(block_len, c["shape"][1], c["shape"][0], c["mode"])

    @staticmethod
    def float_case(c):
        return dict(c, out=0)                                    # the bound is the float32 output's

    @classmethod
    def floats(cls, rng, c, n):
        D, T = c["shape"]
        x = cls.m.float_input(rng, n, c["mode"])
        return x, dict(taps=_lowpass(rng, T, D), x=x)

    @classmethod
    def float_ratio(cls, c, ctx, n, got):
        D, x = c["shape"][0], ctx["x"][:n]
        if "_fwant" not in ctx:                                  # once for the whole input: a shorter stream's outputs are a prefix
            ctx["_fwant"] = cls.m.fir_at(cls.m.detect(ctx["x"], c["mode"]), ctx["taps"], D, 0, cls.m.out_count(0, ctx["n"], D))
        want = ctx["_fwant"][:cls.m.out_count(0, n, D)]
        assert got[0].shape == (1, len(want))
        return float(np.max(np.abs(got[0][0].astype(np.float64) - want), initial=0.0)) / cls.m.bound(ctx["taps"], c["mode"], np.abs(x).max(initial=0.0))

    @classmethod
    def emulate(cls, c, ctx, n):
        D = c["shape"][0]
        return [cls.m.f32_fir(cls.m.f32_detect(ctx["x"][:n], c["mode"]), ctx["taps"], D, 0, cls.m.out_count(0, n, D))[None, :]]

    call = Ddc.call
    call_blocks = Ddc.call_blocks


class Resamp:
    lib, module = "resamp", "resamp"
    import resamp_model as m

    @classmethod
    def create(cls, X, c, ctx, max_in):
        L, M, P = c["shape"]
        return X.Resampler(L, M, ctx["taps"], type="c64" if c["type"] else "f32", out_fmt="s16" if c["out"] else "same",
                           pcm_scale=ctx.get("pcm_scale", 1.0), max_in=max_in)

    @staticmethod
    def hist(c):
        return c["shape"][2] - 1

    @staticmethod
    def in_bytes(c):
        return 8 if c["type"] else 4

    @staticmethod
    def outs(c):
        return [(2 if c["out"] else 8 if c["type"] else 4, 1)]

    @staticmethod
    def dtypes(c):
        return [np.int16 if c["out"] else np.complex64 if c["type"] else np.float32]

    @staticmethod
    def need(c, count):
        return ((count - 1) * c["shape"][1]) // c["shape"][0] + 1

    @classmethod
    def out_count(cls, c, seen, n):
        return cls.m.out_count(seen, n, c["shape"][0], c["shape"][1])

    @classmethod
    def exact(cls, rng, c, n):
        L, M, P = c["shape"]
        taps, num, den = cls.m.exact_taps(rng, L * P, "pow2" if (c["type"] or c["out"]) else "int")
        return cls.m.exact_samples(rng, n, bool(c["type"])), dict(taps=taps, num=num, den=den, pcm_scale=0.25 if c["out"] else 1.0)

    @classmethod
    def exact_want(cls, c, ctx, n):
        L, M, P = c["shape"]
        return [cls.m.exact_stream(ctx["raw"][:n], ctx["num"], ctx["den"], L, M, c["out"], ctx["pcm_scale"])[None, :]]

    @classmethod
    def exact_blocks(cls, c, ctx, starts, block_len):
        L, M, P = c["shape"]
        return [cls.m.exact_blocks(ctx["raw"], ctx["num"], ctx["den"], L, M, starts, block_len, c["out"], ctx["pcm_scale"])]

    @classmethod
    def block_min(cls, c):
        L, M, P = c["shape"]
        return cls.m.block_first(L, M, P) * M // L + 1

    @classmethod
    def block_count(cls, c, block_len):
        return cls.m.block_out_count(block_len, *c["shape"])

    @staticmethod
    def float_case(c):
        return dict(c, out=0)

    @classmethod
    def floats(cls, rng, c, n):
        L, M, P = c["shape"]
        x = rng.uniform(-1, 1, n).astype(np.float32)
        if c["type"]:
            x = (x + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)
        return x, dict(taps=(rng.uniform(-1, 1, L * P) * np.hamming(L * P + 2)[1:-1]).astype(np.float32), x=x)

    @classmethod
    def float_ratio(cls, c, ctx, n, got):
        L, M, P = c["shape"]
        x = ctx["x"][:n]
        ms = np.arange(cls.m.out_count(0, n, L, M))
        want = cls.m.at(x.astype(np.complex128 if c["type"] else np.float64), ctx["taps"].astype(np.float64), L, M, ms)
        assert got[0].shape == (1, len(ms))
        return cls.m.worst_ratio(got[0][0], want, x, ctx["taps"], L, M, ms) if len(ms) else 0.0

    @classmethod
    def emulate(cls, c, ctx, n):
        L, M, P = c["shape"]
        return [cls.m.f32_at(ctx["x"][:n], ctx["taps"], L, M, np.arange(cls.m.out_count(0, n, L, M)))[None, :]]

    call = Ddc.call
    call_blocks = Ddc.call_blocks


class Chan:
    lib, module = "chan", "chan"
    import chan_model as m

    @classmethod
    def create(cls, X, c, ctx, max_in):
        M, O, P = c["shape"]
        return X.Channelizer(c["fmt"], M, O, ctx["taps"], max_in=max_in, u8_offset=128.0, u8_scale=128.0)

    @staticmethod
    def hist(c):
        return c["shape"][0] * c["shape"][2] - 1

    @staticmethod
    def in_bytes(c):
        return SAMPLE_BYTES[c["fmt"]]

    @staticmethod
    def outs(c):
        return [(8, c["shape"][0])]

    @staticmethod
    def dtypes(c):
        return [np.complex64]

    @staticmethod
    def need(c, count):
        return (c["shape"][0] // c["shape"][1]) * (count - 1) + 1

    @classmethod
    def out_count(cls, c, seen, n):
        return cls.m.out_count(seen, n, c["shape"][0] // c["shape"][1])

    @staticmethod
    def axis_channels(c):
        M = c["shape"][0]
        return sorted({0, M // 2} | ({M // 4, 3 * M // 4} if M >= 4 else set()))

    @classmethod
    def exact(cls, rng, c, n):
        M, O, P = c["shape"]
        taps = _int_taps(rng, M * P, 3)
        amp = max(1, min(100, _fmt_amp(c["fmt"]), 2 ** 23 // (3 * M * P)))       # 3 T amp <= 2^23
        raw = _int_raw(rng, c["fmt"], n, amp)
        iq, scale = cls.m.to_int(raw, c["fmt"])
        return raw, dict(taps=taps.astype(np.float32), itaps=taps, iq=iq, scale=scale)

    @classmethod
    def exact_check(cls, c, ctx, n, got, what):
        """The axis channels (0, M/4, M/2, 3M/4: the mixer only takes 1, -i, -1, i there) bit for bit."""
        M, O, P = c["shape"]
        cols = np.arange(cls.m.out_count(0, n, M // O))
        assert got[0].shape == (M, len(cols)), (what, got[0].shape)
        if "_want" not in ctx:                                   # once for the whole input: a shorter stream's columns are a prefix
            every = np.arange(cls.m.out_count(0, ctx["n"], M // O))
            ctx["_want"] = {ch: cls.m.int_channel(ctx["iq"], ctx["scale"], ctx["itaps"], M, O, ch, every) for ch in cls.axis_channels(c)}
        for ch, want in ctx["_want"].items():
            assert np.array_equal(got[0][ch], want[:len(cols)]), (what, "channel", ch)

    @classmethod
    def exact_blocks_check(cls, c, ctx, starts, block_len, got, what):
        M, O, P = c["shape"]
        first, J = cls.m.first_column(M, O, P), cls.block_count(c, block_len)
        for b, lo in enumerate(starts):
            for ch in cls.axis_channels(c):
                want = cls.m.int_channel(ctx["iq"][lo:lo + block_len], ctx["scale"], ctx["itaps"], M, O, ch, np.arange(first, first + J))
                assert np.array_equal(got[0][b * M + ch], want), (what, "block", b, "channel", ch)

    @classmethod
    def block_min(cls, c):
        M, O, P = c["shape"]
        return cls.m.block_len_for(1, M, O, P)

    @classmethod
    def block_count(cls, c, block_len):
        return cls.m.block_out_count(block_len, *c["shape"])

    @staticmethod
    def float_case(c):
        return c

    @classmethod
    def floats(cls, rng, c, n):
        M, O, P = c["shape"]
        raw = _float_raw(rng, c["fmt"], n)
        return raw, dict(taps=_lowpass(rng, M * P, M), x=cls.m.unpack(raw, c["fmt"], 128.0, 128.0))

    @classmethod
    def float_ratio(cls, c, ctx, n, got):
        M, O, P = c["shape"]
        x = ctx["x"][:n]
        want = cls.m.polyphase(x, ctx["taps"], M, O)
        assert got[0].shape == want.shape, (got[0].shape, want.shape)
        return float(np.max(np.abs(got[0] - want), initial=0.0)) / cls.m.bound(ctx["taps"], np.abs(x).max(initial=0.0), M, P) if n else 0.0

    @classmethod
    def emulate(cls, c, ctx, n):
        M, O, P = c["shape"]
        return [cls.m.f32_polyphase(ctx["x"][:n], ctx["taps"], M, O, np.arange(cls.m.out_count(0, n, M // O)))]

    @staticmethod
    def call(obj, c, in_ptr, n, ptrs, cnt, stride):
        return obj.process_dev(in_ptr, n, out=ptrs[0], chan_stride=stride)

    @staticmethod
    def call_blocks(obj, c, in_ptr, nblocks, block_len, block_stride, ptrs, out_stride):
        return obj.blocks_dev(in_ptr, nblocks, block_len, block_stride=block_stride, out=ptrs[0], chan_stride=out_stride)


class Corr:
    lib, module = "corr", "corr"
    import corr_model as m
    THRESHOLD = 0.5

    @classmethod
    def create(cls, X, c, ctx, max_in):
        return X.Correlator(ctx["templates"], threshold=cls.THRESHOLD, guard=c["G"], capacity=c["capacity"], max_in=max_in,
                            fmt=FMT_NAMES[c["fmt"]], u8_offset=128.0, u8_scale=1.0)

    @staticmethod
    def hist(c):
        return c["shape"][0] - 1

    @staticmethod
    def in_bytes(c):
        return SAMPLE_BYTES[c["fmt"]]

    @staticmethod
    def outs(c):
        return [(4, c["shape"][1]), (8, c["shape"][1])]

    @staticmethod
    def dtypes(c):
        return [np.float32, np.complex64]

    @staticmethod
    def need(c, count):
        return count + c["shape"][0] - 1

    @classmethod
    def out_count(cls, c, seen, n):
        return cls.m.out_count(seen, n, c["shape"][0])

    @classmethod
    def exact(cls, rng, c, n):
        """Integer samples and templates in {1, -1, i, -i} with copies of the templates planted.  Up to K = 256 the samples are
        corr_model.exact_samples; beyond, 0, +-1 and +-i with two zeros in five, so that e K and |r|^2 stay below 2^24 (a window
        on a planted copy has e = K, and K^2 < 2^24 up to K = 4095)."""
        K, Q = c["shape"]
        tm = cls.m.exact_templates(rng, Q, K)
        if K <= 256:
            x = cls.m.exact_samples(rng, n)
        else:
            x = np.array([0, 0, 1, -1, 1j], dtype=np.complex64)[rng.integers(0, 5, n)] * np.array([1, 1j], dtype=np.complex64)[rng.integers(0, 2, n)]
        for i in range(3):
            if n >= K + 2 and K < 4096:
                at = int(rng.integers(0, n - K + 1))
                x[at:at + K] = (1 + i % 3 if K <= 256 else 1) * tm[i % Q]
        ints = np.stack([x.real, x.imag], axis=1)
        raw, rscale = {FMT_C64: (x, 1.0), FMT_U8: ((ints + 128).astype(np.uint8), 1.0), FMT_S8: (ints.astype(np.int8), 2.0 ** -7),
                       FMT_S16: (ints.astype(np.int16), 2.0 ** -15)}[c["fmt"]]
        return raw, dict(templates=tm, x=x, rscale=np.float32(rscale))

    @classmethod
    def _model(cls, c, ctx, x):
        rho, r = cls.m.exact_model(x, ctx["templates"])
        return rho, (r * ctx["rscale"]).astype(np.complex64)

    @classmethod
    def exact_want(cls, c, ctx, n):
        return list(cls._model(c, ctx, ctx["x"][:n]))

    @classmethod
    def exact_events(cls, c, ctx, n):
        """(the first `capacity` records, events_total) of the flushed stream of n samples."""
        rho, r = _stream_want(cls, c, ctx, n)
        ev = cls.m.records(rho, r, cls.THRESHOLD, c["G"])
        return ev[:c["capacity"]], len(ev)

    @classmethod
    def exact_blocks(cls, c, ctx, starts, block_len):
        res = [cls._model(c, ctx, ctx["x"][s:s + block_len]) for s in starts]
        return [np.concatenate([a for a, _ in res]), np.concatenate([b for _, b in res])]

    @classmethod
    def exact_block_events(cls, c, ctx, starts, block_len):
        res = [cls._model(c, ctx, ctx["x"][s:s + block_len]) for s in starts]
        ev = cls.m.block_records(np.stack([a for a, _ in res]), np.stack([b for _, b in res]), cls.THRESHOLD, c["G"])
        return ev[:c["capacity"]], len(ev)

    @staticmethod
    def events_equal(a, b):
        return a.dtype == b.dtype and a.shape == b.shape and all(np.array_equal(a[k], b[k]) for k in a.dtype.names)

    @staticmethod
    def block_min(c):
        return c["shape"][0]

    @staticmethod
    def block_count(c, block_len):
        return block_len - c["shape"][0] + 1

    @staticmethod
    def float_case(c):
        return dict(c, fmt=FMT_C64)                              # the bound is written for complex64 samples

    @classmethod
    def floats(cls, rng, c, n):
        K, Q = c["shape"]
        tm = (rng.uniform(-1, 1, (Q, K)) + 1j * rng.uniform(-1, 1, (Q, K))).astype(np.complex64)
        x = _float_raw(rng, FMT_C64, n)
        return x, dict(templates=tm, x=x)

    @classmethod
    def float_ratio(cls, c, ctx, n, got):
        K, Q = c["shape"]
        lags = cls.m.lags_after(n, K)
        assert got[0].shape == got[1].shape == (Q, lags)
        return max(cls.m.worst_ratios(got[0], got[1], ctx["x"][:n], ctx["templates"])) if lags else 0.0

    @classmethod
    def emulate(cls, c, ctx, n):
        return list(cls.m.f32_chain(ctx["x"][:n], ctx["templates"]))

    @staticmethod
    def call(obj, c, in_ptr, n, ptrs, cnt, stride):
        return obj.process_dev(in_ptr, n, metric=ptrs[0], corr=ptrs[1], out_stride=stride)

    @staticmethod
    def call_blocks(obj, c, in_ptr, nblocks, block_len, block_stride, ptrs, out_stride):
        return obj.blocks_dev(in_ptr, nblocks, block_len, block_stride=block_stride, metric=ptrs[0], corr=ptrs[1], out_stride=out_stride)


def _stream_want(cls, c, ctx, n):
    """The exact dense outputs of the stream's first n samples: computed once for the whole input of the case (every model here
    is causal, so a shorter stream's outputs are a prefix) and cut."""
    if "_want" not in ctx:
        ctx["_want"] = cls.exact_want(c, ctx, ctx["n"])
    cnt = cls.out_count(c, 0, n)
    return [w[:, :cnt] for w in ctx["_want"]]


def _exact_check(cls, c, ctx, n, got, what):
    """The default of an adapter: every dense output of the stream's first n samples equals the integer model's value, type and
    shape (np.array_equal, as the libraries' own exact tests compare: an integer model has no sign of zero to give, and the
    float32 chains, the models' emulations included, produce -0 where a negative product is added to nothing)."""
    for g, w in zip(got, _stream_want(cls, c, ctx, n)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), (what, "first differing value", _first_diff(g, w))


def _exact_blocks_check(cls, c, ctx, starts, block_len, got, what):
    want = cls.exact_blocks(c, ctx, starts, block_len)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), (what, "first differing value", _first_diff(g, w))


def _first_diff(g, w):
    bad = np.argwhere(g != w)
    return (tuple(int(v) for v in bad[0]), g[tuple(bad[0])], w[tuple(bad[0])]) if len(bad) else None


for _cls in (Ddc, Demod, Resamp, Corr):
    _cls.exact_check = classmethod(_exact_check)
    _cls.exact_blocks_check = classmethod(_exact_blocks_check)
ADAPTERS = {a.lib: a for a in (Ddc, Demod, Resamp, Chan, Corr)}


def prepare(A, c, n, exact, seed):
    """(raw input of n samples, ctx) of a case from its own seed: exact integers or floats."""
    rng = np.random.default_rng(seed)
    raw, ctx = (A.exact if exact else A.floats)(rng, c, n)
    ctx["raw"], ctx["n"] = raw, n
    return raw, ctx


def block_len_for(A, c, J):
    """The shortest block that yields J outputs (columns, lags) per block."""
    s = c["shape"]
    if A.lib in ("ddc", "demod"):
        return A.block_min(c) + s[0] * (J - 1)
    if A.lib == "resamp":
        return ((A.m.block_first(*s) + J - 1) * s[1]) // s[0] + 1
    if A.lib == "chan":
        return A.m.block_len_for(J, *s)
    return s[0] + J - 1


def edge_streams(A, c, tile):
    """[(prefix, n)] of the streams an edge shape runs: a first call of `prefix` samples, the history (T - 1, P - 1, K - 1)
    rounded up to whole outputs, so that every tap of every later output meets data and the far end of the LDS span holds
    samples, then a call of the fewest n samples that yields tile - 1, tile, tile + 1 and 2 tile + 3 outputs."""
    step = max(1, A.need(c, 2) - A.need(c, 1))
    prefix = -(-A.hist(c) // step) * step
    out = []
    for count in (tile - 1, tile, tile + 1, 2 * tile + 3):
        if count < 1:
            continue
        lo, hi = 1, A.need(c, count + 1) + step + 1               # out_count(prefix, n) does not fall as n grows
        while lo < hi:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if A.out_count(c, prefix, mid) >= count else (mid + 1, hi)
        assert A.out_count(c, prefix, lo) == count, (A.lib, c["shape"], count)
        out.append((prefix, lo))
    return out


def edge_seed(lib, shape, k):
    """The seed of variant k of an edge shape's inputs (the float inputs append 1, the cuts of a stream its length)."""
    return [20201226, LIBS.index(lib), k] + list(shape)


def edge_cuts(A, c, k, n):
    """The cut of the n-sample stream of variant k of an edge shape."""
    return make_cuts(np.random.default_rng(edge_seed(A.lib, c["shape"], k) + [n]), n, A.hist(c))


def max_count(lib, shape, tile):
    """The most outputs (columns, lags) of a stream whose input stays within MAX_IN samples and whose models stay affordable:
    the integer and float64 models cost outputs x taps multiply-adds (ddc, demod, chan, resamp) or lags x K x Q (corr)."""
    A = ADAPTERS[lib]
    c = dict(shape=shape)
    per = {"ddc": lambda: shape[0] * shape[1], "demod": lambda: shape[0] * shape[1], "resamp": lambda: 8 * shape[2] * max(1, shape[1] // shape[0]),
           "chan": lambda: 32 * shape[0] * shape[2], "corr": lambda: shape[0] * shape[1]}[lib]()
    most = max(1, min(3 * tile + 7, (1 << 27) // per))
    while most > 1 and A.need(c, most) > MAX_IN:
        most = most * 3 // 4
    return most


# ------------------------------------------------------------------------------------------ the draws
def _log_int(rng, lo, hi):
    return int(min(hi, max(lo, round(float(np.exp(rng.uniform(np.log(lo), np.log(hi + 0.999))) - 0.5)))))


def _free_shape(lib, rng, type):
    """A shape log-uniform over the library's valid space."""
    if lib in ("ddc", "demod"):
        return (_log_int(rng, 1, limit(lib, "D")), _log_int(rng, 1, limit(lib, "T")))
    if lib == "chan":
        shapes = chan_shapes()
        return shapes[int(rng.integers(0, len(shapes)))]         # M a power of two, O of 1, 2, 4: uniform is log-uniform
    if lib == "corr":
        Q = _log_int(rng, 1, limit(lib, "Q"))
        return (_log_int(rng, 1, min(limit(lib, "K"), limit(lib, "QK") // Q)), Q)
    while True:
        L = _log_int(rng, 1, limit(lib, "L"))
        M = _log_int(rng, 1, min(limit(lib, "M"), limit(lib, "ratio") * L))
        P = _log_int(rng, 1, min(limit(lib, "P"), limit(lib, "T") // L))
        if resamp_valid(L, M, P):
            return (L, M, P)


def _near_shapes(lib, type):
    """[(shape, threshold)] of every valid shape whose varying parameter lies within +-2 of a threshold (last - 1 .. first + 1)."""
    if lib == "resamp":
        cr = [((L, M, P), 2) for L, v in sorted(resamp_crossings(type).items()) for M, P in v]
    elif lib == "corr":
        q_max, r_small, r_large = corr_lag_rule()
        cr = [((K, q_max), 1) for K in (1, 7, 64, 300, 1500, 4096)]
        cr += [((c * R, Q), 0) for Q, R in ((1, r_small), (2, r_small), (3, r_large), (8, r_large)) for c in (1, 2, 9, 40, 200, 500)]
    else:
        cr = crossings(lib)
    out = []
    for last, vary in cr:
        for delta in (-1, 0, 1, 2):
            s = tuple(v + (delta if i == vary else 0) for i, v in enumerate(last))
            if valid(lib, s):
                out.append((s, last))
    return out


_NEAR = {}


def _shape_for(lib, rng, key, near, type):
    """A shape whose plan is `key`: near a threshold if asked and the plan borders one, else log-uniform."""
    if near:
        if (lib, type) not in _NEAR:
            _NEAR[(lib, type)] = _near_shapes(lib, type)
        cands = [s for s, _ in _NEAR[(lib, type)] if plan_key(lib, plan_of(lib, s, type), type) == key]
        if cands:
            return cands[int(rng.integers(0, len(cands)))], True
    for _ in range(100000):
        s = _free_shape(lib, rng, type)
        if plan_key(lib, plan_of(lib, s, type), type) == key:
            return s, False
    raise AssertionError("no shape of plan %s %s found" % (lib, key))


def _draw_plan_case(lib, i, rng):
    A = ADAPTERS[lib]
    c = dict(lib=lib, i=i, seed=int(rng.integers(1, 2 ** 31)))
    if lib in ("ddc", "chan", "corr"):
        c["fmt"] = FMTS[i % 4]
    if lib == "ddc":
        c["quarter"] = int(rng.integers(0, 4))
    if lib == "demod":
        c["mode"], c["out"] = (i % 6) % 3, (i % 6) // 3
    if lib == "resamp":
        c["type"], c["out"] = [(0, 0), (1, 0), (0, 1)][i % 3]
    type = c.get("type", 0)
    plans = sorted(k for k in all_plans(lib) if lib != "resamp" or k[0] == type)
    key = plans[(i // 3 if lib == "resamp" else i + i // len(plans)) % len(plans)]
    c["shape"], c["near"] = _shape_for(lib, rng, key, i % 2 == 1, type)
    if lib == "corr":
        K = c["shape"][0]
        c["G"] = int(rng.choice([1, 5, K]))
        c["capacity"] = int(rng.choice([2, 4096]))               # 2: fewer than the planted copies' records
    tile = tile_of(plan_of(lib, c["shape"], type))
    most = max_count(lib, c["shape"], tile)
    c["count"] = int(rng.integers(1, most + 1)) if most < tile + 2 or rng.random() < 0.3 else int(rng.integers(tile, most + 1))
    step = A.need(c, 2) - A.need(c, 1)
    c["n"] = min(MAX_IN, A.need(c, c["count"]) + int(rng.integers(0, max(1, step))))
    c["cuts"] = make_cuts(rng, c["n"], A.hist(c))
    per16 = 16 // A.in_bytes(c)
    c["offset"] = 0 if i % 3 == 0 else int(rng.integers(1, per16))
    c["out_offset"] = i % 2                                      # values from 16-byte alignment
    J = int(rng.integers(1, max(2, min(most, tile + 3))))
    bl = block_len_for(A, c, J) + int(rng.integers(0, 3))
    nblocks = int(rng.integers(1, 5))
    stride = [0, max(1, bl // 2), bl, bl + 5][(i // 2) % 4]
    c["block"] = dict(nblocks=nblocks, block_len=bl, block_stride=stride, out_pad=3 * (i % 2), J=A.block_count(c, bl))
    return c


# -- the list libraries: density, mask, detect (rows of a spectrum), track (a list of spans), pulse, iqfix (raw IQ) --------------
def _nbins(rng, i, lo, hi):
    """The header's minimum, a power of two, or a value that is none (odd), log-uniform."""
    if i % 4 == 0:
        return lo
    n = _log_int(rng, lo, hi)
    return 1 << (n.bit_length() - 1) if i % 4 == 1 else min(hi, n | 1)


def _split(rng, total, parts):
    """`parts` positive counts that sum to total (fewer when total is smaller)."""
    parts = min(parts, total)
    at = np.sort(rng.choice(np.arange(1, total), parts - 1, replace=False)) if parts > 1 else np.zeros(0, dtype=np.int64)
    return [int(v) for v in np.diff(np.concatenate([[0], at, [total]]))]


def _draw_list_case(lib, i, rng):
    c = dict(lib=lib, i=i, seed=int(rng.integers(1, 2 ** 31)))
    if lib in ("density", "mask", "detect"):
        lo = header_constant("ksa_%s.h" % lib, {"density": "KSD", "mask": "KSM", "detect": "KSE"}[lib] + "_MIN_NBINS")
        hi = min(1 << 17, header_constant("ksa_%s.h" % lib, {"density": "KSD", "mask": "KSM", "detect": "KSE"}[lib] + "_MAX_NBINS"))
        c["nbins"] = nbins = _nbins(rng, i, lo, hi)
        cells = MAX_CELLS if lib != "detect" else MAX_CELLS // 4  # the detector's model walks its rows one by one
        c["rows"] = _split(rng, int(rng.integers(3, max(4, min(300, cells // nbins) + 1))), 2 + i % 2)
        c["row_stride"] = nbins + [0, 1, 5, 64][(i // 2) % 4]
        c["base"] = i % 2                                        # floats from 16-byte alignment
        if lib == "density":
            divisors = [d for d in range(1, min(nbins, 4096) + 1) if nbins % d == 0] + [nbins]
            c["width"] = int(rng.choice(divisors)) if i % 3 else nbins
            c["levels"] = [1, header_constant("ksa_density.h", "KSD_MAX_LEVELS"), _log_int(rng, 2, 1023)][i % 3]
            c["lo_db"], c["hi_db"] = [(-140.0, 0.0), (-100.5, -20.25)][(i // 3) % 2]
            c["decay"] = (3, 4) if i % 4 == 2 else None
        elif lib == "mask":
            c["lower"] = bool(i % 2)
            c["min_bins"] = [1, 3, nbins][i % 3]
            c["capacity"] = [2, 4096][(i // 2) % 2]
            c["row_base"] = [0, 2 ** 33][(i // 4) % 2]
        else:
            c["train"], c["guard"] = [(_log_int(rng, 1, 64), _log_int(rng, 1, 8)), (1024, 256), (1, 0), (_log_int(rng, 1, 1024), 0)][i % 4]
            c["mode"] = i % 3
            c["min_width"] = [1, 3, 2][(i // 3) % 3]
            c["max_gap"] = [0, 2, 1024][(i // 2) % 3]
            c["capacity"] = [3, 1 << 16][(i // 2) % 2]
            c["row_base"] = [0, 2 ** 33][(i // 4) % 2]
    elif lib == "track":
        c["occ_rows"], c["occ_bins"] = int(rng.integers(3, 120)), int(rng.choice([1, 8, 64, 333]))
        c["p"] = float(rng.uniform(0.05, 0.3))
        c["nbins"] = [c["occ_bins"], 1 << 24][i % 2]
        c["row_gap"] = [0, 2, header_constant("ksa_track.h", "KTR_MAX_ROW_GAP")][i % 3]
        c["bin_slop"] = min([0, 1, 5][(i // 3) % 3], c["nbins"])  # the header refuses a slop beyond nbins
        c["min_rows"], c["min_spans"] = [(1, 1), (3, 1), (1, 4), (2, 2)][i % 4]
        c["capacity"] = [2, 4096][(i // 2) % 2]
        c["extra"] = [0, 7][i % 2]                               # records behind the count on the device, which must not be read
        c["row0"] = [0, 2 ** 40][(i // 4) % 2]
    else:                                                        # pulse, iqfix
        c["fmt"] = FMTS[i % 4]
        c["offset"] = 0 if i % 3 == 0 else int(rng.integers(1, 16 // SAMPLE_BYTES[c["fmt"]]))
        if lib == "pulse":
            c["W"] = [1, header_constant("ksa_pulse.h", "KPL_MAX_W"), _log_int(rng, 2, 4095)][i % 3]
            c["min_len"] = [1, 5, 50][(i // 3) % 3]
            c["capacity"] = [2, 4096][(i // 2) % 2]
            c["n"] = int(rng.integers(3 * c["W"] + 10, min(1 << 16, 20 * c["W"] + 4000)))
            c["cuts"] = make_cuts(rng, c["n"], c["W"] - 1)
        else:
            c["mode"] = [1, 2, 3][i % 3]
        calls = []
        for k in range(2 + i % 2 if lib == "iqfix" else 1):
            bl = int(rng.integers(1, 3000))
            calls.append(dict(nblocks=int(rng.integers(1, 5)), block_len=bl, block_stride=[0, max(1, bl // 2), bl, bl + 5][(i // 2 + k) % 4],
                              out_pad=3 * ((i + k) % 2), accumulate=(i + k) % 3 != 2))
        c["blocks"] = calls
    return c


def rows_input(c):
    """(float32 [sum(rows)][nbins], extras) of a density, mask or detect case: the cloud of the library's own GPU file, which
    holds infinities, NaN and values on and one ulp either side of every edge."""
    total, nbins = sum(c["rows"]), c["nbins"]
    if c["lib"] == "density":
        from test_gpu_density import cloud
        return cloud(c["seed"], total, nbins, c["levels"], c["lo_db"], c["hi_db"]), {}
    if c["lib"] == "mask":
        from test_gpu_mask import cloud, lines_for
        up, lo = lines_for(nbins, c["lower"])
        return cloud(c["seed"], total, nbins, up, lo), dict(upper=up, lower=lo)
    from test_gpu_detect import cloud
    return cloud(c["seed"], total, nbins), {}


def strided_rows(rows, stride, base):
    """float32 [base + k * stride]: the rows `stride` floats apart behind `base` floats, NaN everywhere between them (a NaN
    that a kernel read would be counted by every one of the three libraries)."""
    k, nbins = rows.shape
    out = np.full(base + k * stride, np.nan, dtype=np.float32)
    view = out[base:].reshape(k, stride)
    view[:, :nbins] = rows
    return out


def track_input(c):
    """SPAN_DTYPE records of a track case (track_model.random_occupancy) and the row_end that goes with them."""
    import track_model as tm
    spans = tm.random_occupancy(c["occ_rows"], c["occ_bins"], c["p"], c["seed"], c["row0"])
    return spans, c["row0"] + c["occ_rows"] + (c["i"] % 3) * (c["row_gap"] + 1)


def bursty_raw(rng, fmt, n):
    """Raw IQ of n samples in the format: noise near -40 dBFS with bursts near -6 dBFS of 1 .. 600 samples, some of them
    clipping; complex64 [n] or integers [n][2]."""
    x = 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    at = 0
    while at < n:
        at += int(rng.integers(1, 900))
        ln = int(rng.integers(1, 600))
        x[at:at + ln] += rng.uniform(0.2, 1.2) * np.exp(2j * np.pi * (rng.uniform() + 0.01 * np.arange(len(x[at:at + ln]))))
        at += ln
    if fmt == FMT_C64:
        return x.astype(np.complex64)
    full, dtype = {FMT_U8: (127.5, np.uint8), FMT_S8: (128.0, np.int8), FMT_S16: (32768.0, np.int16)}[fmt]
    v = np.stack([x.real, x.imag], axis=1) * full + (127.5 if fmt == FMT_U8 else 0.0)
    info = np.iinfo(dtype)
    return np.clip(np.rint(v), info.min, info.max).astype(dtype)


def draw(lib, count, seed):
    """`count` seeded cases of the library (dicts; the GPU test runs them, the host test holds them to the coverage conditions).
    Case i aims at plan i mod the number of plans and cycles through the formats, modes and types, so that a default draw
    reaches all of them; the shapes with even i are log-uniform over the valid space, those with odd i lie within +-2 of a
    threshold in the varying parameter wherever the plan borders one."""
    rng = np.random.default_rng([seed, LIBS.index(lib)])
    if lib in PLAN_LIBS:
        return [_draw_plan_case(lib, i, rng) for i in range(count)]
    return [_draw_list_case(lib, i, rng) for i in range(count)]


def case_id(c):
    keys = ("shape", "fmt", "mode", "type", "out", "nbins", "rows")
    return "%s-%d-%s" % (c["lib"], c["i"], "-".join("%s%s" % (k[0], str(c[k]).replace(" ", "")) for k in keys if k in c))
