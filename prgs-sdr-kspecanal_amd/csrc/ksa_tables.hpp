// Host-side table builders of libksa: the twiddle and tap tables the kernels read, and the plan of the mixed-radix path.
// Pure functions of sizes: no HIP call, no engine.  ksa_create (ksa_api.hip) uploads what they return.
// Angles are computed in double and stored as float.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "ksa_kernels_mr.hpp"

namespace ksa {
namespace tables {

inline float2 cis(double ang) { return make_float2((float)std::cos(ang), (float)std::sin(ang)); }

// Entry e = 0..14 of the folded twiddles of dft16_fused for a base twiddle w of `beta` turns: w^4, w^8, w^12, then
// c[n2][k1] = w^n2 * W16^(n2*k1) for k1 = 0..3, n2 = 1..3.
inline float2 fused15(double beta, int e) {
  double turns;
  if (e < 3) turns = 4.0 * (e + 1) * beta;
  else { const int k1 = (e - 3) / 3, n2 = (e - 3) % 3 + 1; turns = n2 * beta + (double)(n2 * k1) / 16.0; }
  return cis(-2.0 * M_PI * turns);
}

struct Twiddles {
  std::vector<float2> mid, last;   // d_tw_mid, d_tw_last
};

// The 16-point plan (ksa::Plan<sn>): 16 points per thread, radix-16 passes (an 8-point / radix-8 plan measured 20 % slower).
// Middle passes [15][p] each, last pass [15][sn/16]; `fused_*` (ksa::Tune<sn>::FUSED / FUSED_LAST) picks the rows of
// dft16_fused over the 6-twiddle form's W_(16p)^(t*k), t = 1..15.
inline Twiddles twiddles16(int sn, bool fused_mid, bool fused_last) {
  const int pt = 16, lpt = 4;
  const int log2n = ilog2(sn);
  const int m = (log2n + lpt - 1) / lpt;
  int pcur = 1 << (log2n - lpt * (m - 1));
  Twiddles tw;
  for (int s = 1; s < m; ++s) {
    std::vector<float2>& dst = s < m - 1 ? tw.mid : tw.last;
    if (s < m - 1 ? fused_mid : fused_last) {
      for (int e = 0; e < 15; ++e)
        for (int k = 0; k < pcur; ++k) dst.push_back(fused15((double)k / ((double)pcur * 16.0), e));
    } else {
      for (int t = 1; t < pt; ++t)
        for (int k = 0; k < pcur; ++k) dst.push_back(cis(-2.0 * M_PI * (double)t * (double)k / ((double)pcur * pt)));
    }
    pcur *= pt;
  }
  return tw;
}

// The 32-point plan (ksa::Plan32<sn>, sn = 8192 or 16384): one middle pass at p = 32, then the last pass.
inline Twiddles twiddles32(int sn) {
  const int lth = sn / 32;
  Twiddles tw;
  if (sn == 16384) {       // middle pass radix 32, p = 32: [31][32] = w^16 | fused15(k/1024) | fused15(k/1024 + 1/32)
    tw.mid.resize((size_t)31 * 32);
    for (int k = 0; k < 32; ++k) {
      const double beta = (double)k / 1024.0;
      tw.mid[k] = cis(-2.0 * M_PI * 16.0 * beta);
      for (int e = 0; e < 15; ++e) {
        tw.mid[(size_t)(1 + e) * 32 + k] = fused15(beta, e);
        tw.mid[(size_t)(16 + e) * 32 + k] = fused15(beta + 1.0 / 32.0, e);
      }
    }
  } else {                 // middle pass radix 16, p = 32: [15][32] = fused15(k/512)
    tw.mid.resize((size_t)15 * 32);
    for (int k = 0; k < 32; ++k)
      for (int e = 0; e < 15; ++e) tw.mid[(size_t)e * 32 + k] = fused15((double)k / 512.0, e);
  }
  // last pass radix 16, two butterflies per thread, k = i = l + b*L: [(b*15 + e)][L]
  tw.last.resize((size_t)30 * lth);
  for (int b = 0; b < 2; ++b)
    for (int e = 0; e < 15; ++e)
      for (int l = 0; l < lth; ++l) tw.last[(size_t)(b * 15 + e) * lth + l] = fused15((double)(l + b * lth) / (double)sn, e);
  return tw;
}

// The 8 x 8 plan of N = 64 (ksa_kernels64.hpp): W64^(m k1) as [m][k1].
inline std::vector<float2> twiddles64() {
  std::vector<float2> tw(64);
  for (int m = 0; m < 8; ++m)
    for (int k1 = 0; k1 < 8; ++k1) tw[(size_t)m * 8 + k1] = cis(-2.0 * M_PI * (double)(m * k1) / 64.0);
  return tw;
}

// Taps in the 32-point kernel's load order (16-byte tap loads, ksa_kernels32.hpp): [q4][l][j] = w[l + L*(4*q4 + j)], L = sn/32.
// window == nullptr: the all-ones table of a transform behind a first stage.
inline std::vector<float> taps32(int sn, const float* window) {
  const int lth = sn / 32;
  std::vector<float> w32((size_t)sn);
  for (int q4 = 0; q4 < 8; ++q4)
    for (int l = 0; l < lth; ++l)
      for (int j = 0; j < 4; ++j) w32[((size_t)q4 * lth + l) * 4 + j] = window ? window[l + lth * (4 * q4 + j)] : 1.0f;
  return w32;
}

// First stage of N > 16384 (ksa_dif16.hpp), n1 = n / radix: output twiddles W_n^(k*e) as [rows][n1], e = 1,2,3,4,8,12
// (radix 16: w^k2 = w^(k2&3) * w^(k2&12)), then 16,32,48 for radix 32 / 64.
inline std::vector<float2> first_stage_twiddles(int n, int radix) {
  static const int ex[9] = {1, 2, 3, 4, 8, 12, 16, 32, 48};
  const int n1 = n / radix, nrows = radix == 16 ? 6 : 9;
  std::vector<float2> tw((size_t)nrows * n1);
  for (int r = 0; r < nrows; ++r)
    for (int k = 0; k < n1; ++k) tw[(size_t)r * n1 + k] = cis(-2.0 * M_PI * (double)ex[r] * (double)k / (double)n);
  return tw;
}

inline int mr_nb(int radix) { return radix == 2 ? MrNb<2>::value : radix == 3 ? MrNb<3>::value : radix == 4 ? MrNb<4>::value : MrNb<5>::value; }

// Plan of path 6: radix-5 passes, radix-3 passes, radix-4 passes, one radix-2 pass if the power of two is odd, and the radix-4
// pass that every plan ends with (N % 4 == 0).  Pass s with ns = product of the radices before it holds
// [R-1][ns] = W_(ns*R)^(r*k), r = 1..R-1, k < ns.  Threads: the fewest (a multiple of 64) that keep every pass at
// ceil(N / (R*T)) <= MrNb<R> butterflies per thread.  Returns the error text, empty when the plan stands (plan->tw stays null).
inline std::string plan_mr(int n, MrPlan* plan, int* threads, std::vector<float2>* tw) {
  int m = n / 4, a = 0, b = 0, c = 0;
  while (m % 2 == 0) { m /= 2; ++a; }
  while (m % 3 == 0) { m /= 3; ++b; }
  while (m % 5 == 0) { m /= 5; ++c; }
  if (m != 1) return "fft_size " + std::to_string(n) + " is not 4 * 2^a * 3^b * 5^c";
  std::vector<int> r;
  r.insert(r.end(), c, 5);
  r.insert(r.end(), b, 3);
  r.insert(r.end(), a / 2, 4);
  if (a % 2) r.push_back(2);
  r.push_back(4);
  if ((int)r.size() > MR_MAX_PASSES) return "fft_size " + std::to_string(n) + " needs " + std::to_string(r.size()) + " passes (> " + std::to_string(MR_MAX_PASSES) + ")";
  *plan = MrPlan{};
  plan->n = n;
  plan->npass = (int)r.size();
  tw->clear();
  int ns = 1;
  for (int s = 0; s < plan->npass; ++s) {
    const int R = r[s];
    plan->radix[s] = R;
    plan->tw_off[s] = (int)tw->size();
    if (s > 0)
      for (int q = 1; q < R; ++q)
        for (int k = 0; k < ns; ++k) tw->push_back(cis(-2.0 * M_PI * (double)q * (double)k / ((double)ns * R)));
    ns *= R;
  }
  for (int t = 64; t <= MR_MAX_THREADS; t += 64) {
    bool fits = true;
    for (int R : r) fits &= (n / R + t - 1) / t <= mr_nb(R);
    if (fits) { *threads = t; return {}; }
  }
  return "fft_size " + std::to_string(n) + " needs more than " + std::to_string(MR_MAX_THREADS) + " threads";
}

}  // namespace tables
}  // namespace ksa
