"""The host-side table builders (csrc/ksa_tables.hpp) against float64 formulas written out here (CPU suite).

A small driver that includes the header is compiled once with hipcc and run once: it makes no HIP call, so it needs no GPU.
It dumps every table as raw float32 (plans as int32).  Tolerance: one float32 ulp at 1.0 (2^-23 = 1.2e-7, absolute) -- every
entry is a cosine or a sine, so it lies in [-1, 1], and both sides round a float64 cos / sin whose last bit may differ
between libm and numpy.  Integer outputs compare exactly."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prgs-sdr-kspecanal_amd", "csrc")
ULP = 2.0 ** -23
MR_SIZES = (20, 96, 2400, 15360)
MR_NB = {2: 8, 3: 6, 4: 4, 5: 4}          # ksa::MrNb<R>: butterflies per thread and pass

DRIVER = r"""
#include "%s"
#include <cstdio>
#include <string>
namespace tab = ksa::tables;
static std::string dir;
template <class T>
static void dump(const std::string& name, const std::vector<T>& v) {
  FILE* f = fopen((dir + "/" + name).c_str(), "wb");
  fwrite(v.data(), sizeof(T), v.size(), f);
  fclose(f);
}
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  dir = argv[1];
  for (int sn : {64, 256, 4096, 8192}) {
    const tab::Twiddles t = tab::twiddles16(sn, sn <= 4096, sn <= 4096);
    dump("tw16_mid_" + std::to_string(sn), t.mid);
    dump("tw16_last_" + std::to_string(sn), t.last);
  }
  for (int sn : {8192, 16384}) {
    const tab::Twiddles t = tab::twiddles32(sn);
    dump("tw32_mid_" + std::to_string(sn), t.mid);
    dump("tw32_last_" + std::to_string(sn), t.last);
  }
  dump("tw64", tab::twiddles64());
  std::vector<float> ramp(8192);
  for (int i = 0; i < 8192; ++i) ramp[i] = (float)i;
  dump("taps32_ramp", tab::taps32(8192, ramp.data()));
  dump("taps32_ones", tab::taps32(8192, nullptr));
  for (int radix : {16, 32, 64}) dump("dif_" + std::to_string(radix), tab::first_stage_twiddles(2048 * radix, radix));
  for (int n : {%s}) {
    ksa::MrPlan plan;
    int threads = 0;
    std::vector<float2> tw;
    if (!tab::plan_mr(n, &plan, &threads, &tw).empty()) return 3;
    std::vector<int> p = {plan.n, plan.npass, threads};
    p.insert(p.end(), plan.radix, plan.radix + plan.npass);
    p.insert(p.end(), plan.tw_off, plan.tw_off + plan.npass);
    dump("mr_plan_" + std::to_string(n), p);
    dump("mr_tw_" + std::to_string(n), tw);
  }
  ksa::MrPlan plan;
  int threads = 0;
  std::vector<float2> tw;
  return tab::plan_mr(28, &plan, &threads, &tw) == "fft_size 28 is not 4 * 2^a * 3^b * 5^c" ? 0 : 4;
}
"""


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    d = tmp_path_factory.mktemp("tables")
    src = d / "tables_driver.hip"
    src.write_text(DRIVER % (os.path.join(CSRC, "ksa_tables.hpp"), ", ".join(str(n) for n in MR_SIZES)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-o", str(d / "tables_driver"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = d / "out"
    out.mkdir()
    r = subprocess.run([str(d / "tables_driver"), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])

    def load(name, dtype=np.float32):
        return np.fromfile(str(out / name), dtype=dtype)
    return load


def w(turns):
    """exp(-2 pi i turns) as interleaved (cos, sin) float64, flattened in C order."""
    ang = -2.0 * np.pi * np.asarray(turns, dtype=np.float64)
    return np.stack([np.cos(ang), np.sin(ang)], axis=-1).reshape(-1)


def close(got, want):
    assert got.dtype == np.float32 and got.shape == want.shape, (got.shape, want.shape)
    assert np.all(np.abs(want) <= 1.0)
    err = np.max(np.abs(got.astype(np.float64) - want)) if want.size else 0.0
    assert err <= ULP, err


# rows of dft16_fused: w^4, w^8, w^12, then w^n2 * W16^(n2*k1) with k1 = 0..3 outer, n2 = 1..3 inner: (power of w, extra turns)
FUSED_ROWS = [(4, 0.0), (8, 0.0), (12, 0.0)] + [(n2, n2 * k1 / 16.0) for k1 in range(4) for n2 in (1, 2, 3)]


def fused(base):
    """[15][len(base)] turns for base twiddles of `base` turns."""
    base = np.asarray(base, dtype=np.float64)
    return np.stack([m * base + x for m, x in FUSED_ROWS])


def passes16(sn):
    """p of passes 1 .. M-1 of the 16-point plan: first-pass radix R0 = sn / 16^(M-1), then times 16 per pass."""
    log2n = sn.bit_length() - 1
    m = (log2n + 3) // 4
    r0 = 1 << (log2n - 4 * (m - 1))
    return [r0 * 16 ** (s - 1) for s in range(1, m)]


@pytest.mark.parametrize("sn", [64, 256, 4096, 8192])
def test_tables_of_the_16_point_plan(tables, sn):
    """Passes 1 .. M-1, each [15][p] over W_(16p): the fused rows up to 4096, W^(t*k) with t = 1..15 at 8192 (the 6-twiddle
    form's table).  64 and 256 have no middle pass."""
    ps = passes16(sn)
    assert ps == {64: [4], 256: [16], 4096: [16, 256], 8192: [2, 32, 512]}[sn]

    def table(p):
        k = np.arange(p, dtype=np.float64)
        if sn <= 4096:
            return w(fused(k / (16.0 * p)))
        return w(np.outer(np.arange(1, 16), k) / (16.0 * p))
    mid = [table(p) for p in ps[:-1]]
    close(tables("tw16_mid_%d" % sn), np.concatenate(mid) if mid else np.zeros(0))
    close(tables("tw16_last_%d" % sn), table(ps[-1]))


@pytest.mark.parametrize("sn", [8192, 16384])
def test_tables_of_the_32_point_plan(tables, sn):
    k = np.arange(32, dtype=np.float64)
    if sn == 16384:      # radix-32 middle pass over W_1024: w^16, the fused rows of w, the fused rows of w * W_32
        mid = np.concatenate([16.0 * k[None, :] / 1024.0, fused(k / 1024.0), fused(k / 1024.0 + 1.0 / 32.0)])
        assert mid.shape == (31, 32)
    else:                # radix-16 middle pass over W_512
        mid = fused(k / 512.0)
    close(tables("tw32_mid_%d" % sn), w(mid))
    lth = sn // 32       # last pass: butterflies l and l + L of a thread, [b][15][L]
    last = np.concatenate([fused((np.arange(lth) + b * lth) / float(sn)) for b in range(2)])
    assert last.shape == (30, lth)
    close(tables("tw32_last_%d" % sn), w(last))


def test_the_8_by_8_table_of_n_64(tables):
    close(tables("tw64"), w(np.outer(np.arange(8), np.arange(8)) / 64.0))


def test_tap_reorder_of_the_32_point_plan(tables):
    """[q4][l][j] = w[l + L*(4*q4 + j)], L = N/32, on a ramp: the entry is its own source index."""
    lth = 8192 // 32
    q4, l, j = np.meshgrid(np.arange(8), np.arange(lth), np.arange(4), indexing="ij")
    want = (l + lth * (4 * q4 + j)).reshape(-1)
    got = tables("taps32_ramp")
    assert np.array_equal(got, want.astype(np.float32)) and sorted(got.tolist()) == list(range(8192))
    assert np.array_equal(tables("taps32_ones"), np.ones(8192, dtype=np.float32))


@pytest.mark.parametrize("radix", [16, 32, 64])
def test_first_stage_twiddle_rows(tables, radix):
    """W_N^(e*k), k < n1 = N / radix = 2048: six rows for radix 16, nine for radix 32 / 64."""
    exps = [1, 2, 3, 4, 8, 12] + ([] if radix == 16 else [16, 32, 48])
    close(tables("dif_%d" % radix), w(np.outer(exps, np.arange(2048)) / (2048.0 * radix)))


@pytest.mark.parametrize("n", MR_SIZES)
def test_mixed_radix_plan(tables, n):
    m, count = n // 4, {}
    for f in (2, 3, 5):
        count[f] = 0
        while m % f == 0:
            m //= f
            count[f] += 1
    assert m == 1
    radix = [5] * count[5] + [3] * count[3] + [4] * (count[2] // 2) + [2] * (count[2] % 2) + [4]
    assert radix == {20: [5, 4], 96: [3, 4, 2, 4], 2400: [5, 5, 3, 4, 2, 4], 15360: [5, 3, 4, 4, 4, 4, 4]}[n]
    tw_off, tw, ns = [], [], 1
    for s, r in enumerate(radix):
        tw_off.append(sum(t.size for t in tw) // 2)
        if s > 0:
            tw.append(w(np.outer(np.arange(1, r), np.arange(ns)) / float(ns * r)))
        ns *= r
    assert ns == n
    threads = next(t for t in range(64, 1025, 64) if all(-(-n // (r * t)) <= MR_NB[r] for r in radix))
    got = tables("mr_plan_%d" % n, np.int32).tolist()
    assert got == [n, len(radix), threads] + radix + tw_off
    close(tables("mr_tw_%d" % n), np.concatenate(tw))
