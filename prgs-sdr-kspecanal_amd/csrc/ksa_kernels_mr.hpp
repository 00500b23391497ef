// Mixed-radix spectrum stage (path 6): fft_size N = 2^a * 3^b * 5^c, a multiple of 4, 16 <= N <= 16384, not a power of two.
//
//  mixed_radix_kernel<FMT>  the contract of spectrum_kernel (same SpecParams, same outputs): unpack, window, N-point FFT, |X|,
//                           fold over the block's windows, scale, fftshift, dB, waterfall cell.  One workgroup per frame
//                           (persistent, grid-stride over frames); the whole transform lives in LDS (N * 8 bytes).
//
// The transform is a Stockham autosort FFT whose passes are decided at run time (MrPlan, built by ksa_create): pass s of radix R
// with ns = product of the radices before it takes butterfly j < N/R from elements j + r*N/R, multiplies element r by
// W_(ns*R)^(r*(j mod ns)), runs an R-point DFT and stores output r at (j - j mod ns)*R + (j mod ns) + r*ns.  The output is in
// natural order.  Pass 0 (ns = 1, no twiddles) reads the windowed samples straight from global memory; the last pass is always
// radix 4 (N % 4 == 0), so butterfly j of a thread ends holding bins j + r*N/4 in registers and the fold runs there, without
// an LDS round trip.  Between passes the data go through LDS once: read, compute, barrier, write, barrier.
//
// Every thread owns at most MrNb<R> butterflies of a radix-R pass (compile-time bounds, predicated: no scratch memory); the host
// picks the thread count so that ceil(N / (R*T)) <= MrNb<R> for every pass of the plan.  Twiddles are host-generated in float64
// and read as float2 through the L1 / L2 caches: pass s's table is [R-1][ns] at plan.tw + plan.tw_off[s].
#pragma once
#include "ksa_kernels.hpp"

namespace ksa {

constexpr int MR_MAX_PASSES = 12;     // N <= 16384 with radices 2 (at most once), 3, 4, 5: at most 10 passes
constexpr int MR_MAX_THREADS = 1024;

struct MrPlan {
  int n;                          // fft_size
  int npass;                      // passes, the last one radix 4
  int radix[MR_MAX_PASSES];       // radix of pass s: 2, 3, 4 or 5
  int tw_off[MR_MAX_PASSES];      // float2 offset of pass s's [radix-1][ns] twiddle table (pass 0 has none)
  const float2* tw;
};

// butterflies per thread and pass: at most 16..20 complex values in registers, whatever the radix
template <int R>
struct MrNb { static constexpr int value = R == 2 ? 8 : R == 3 ? 6 : 4; };

template <int R>
__device__ __forceinline__ void mr_dft(float2 (&v)[R]) {
  if constexpr (R == 2) {
    const float2 a = v[0], b = v[1];
    v[0] = cadd(a, b);
    v[1] = csub(a, b);
  } else if constexpr (R == 3) {
    constexpr float c = -0.5f, s = -0.86602540378443864676f;       // W3 = c + i s
    const float2 a = v[0], t = cadd(v[1], v[2]), u = csub(v[1], v[2]);
    const float2 m = make_float2(fmaf(c, t.x, a.x), fmaf(c, t.y, a.y));
    v[0] = cadd(a, t);
    v[1] = make_float2(fmaf(-s, u.y, m.x), fmaf(s, u.x, m.y));       // m + i s u
    v[2] = make_float2(fmaf(s, u.y, m.x), fmaf(-s, u.x, m.y));       // m - i s u
  } else if constexpr (R == 4) {
    const float2 s0 = cadd(v[0], v[2]), d0 = csub(v[0], v[2]), s1 = cadd(v[1], v[3]), d1 = csub(v[1], v[3]);
    v[0] = cadd(s0, s1);
    v[2] = csub(s0, s1);
    v[1] = make_float2(d0.x + d1.y, d0.y - d1.x);                    // d0 - i d1
    v[3] = make_float2(d0.x - d1.y, d0.y + d1.x);                    // d0 + i d1
  } else {
    static_assert(R == 5, "radix 2, 3, 4 or 5");
    constexpr float c1 = 0.30901699437494742410f, c2 = -0.80901699437494742410f;   // cos(2 pi/5), cos(4 pi/5)
    constexpr float s1 = 0.95105651629515357212f, s2 = 0.58778525229247312917f;    // sin(2 pi/5), sin(4 pi/5)
    const float2 a = v[0];
    const float2 t1 = cadd(v[1], v[4]), u1 = csub(v[1], v[4]), t2 = cadd(v[2], v[3]), u2 = csub(v[2], v[3]);
    const float2 m1 = make_float2(fmaf(c2, t2.x, fmaf(c1, t1.x, a.x)), fmaf(c2, t2.y, fmaf(c1, t1.y, a.y)));
    const float2 m2 = make_float2(fmaf(c1, t2.x, fmaf(c2, t1.x, a.x)), fmaf(c1, t2.y, fmaf(c2, t1.y, a.y)));
    const float2 n1 = make_float2(fmaf(s2, u2.x, s1 * u1.x), fmaf(s2, u2.y, s1 * u1.y));    // s1 u1 + s2 u2
    const float2 n2 = make_float2(fmaf(-s1, u2.x, s2 * u1.x), fmaf(-s1, u2.y, s2 * u1.y));  // s2 u1 - s1 u2
    v[0] = make_float2(a.x + t1.x + t2.x, a.y + t1.y + t2.y);
    v[1] = make_float2(m1.x + n1.y, m1.y - n1.x);                    // m1 - i n1
    v[4] = make_float2(m1.x - n1.y, m1.y + n1.x);                    // m1 + i n1
    v[2] = make_float2(m2.x + n2.y, m2.y - n2.x);                    // m2 - i n2
    v[3] = make_float2(m2.x - n2.y, m2.y + n2.x);                    // m2 + i n2
  }
}

// Pass 0: windowed samples start + j + r*N/R of the frame -> R-point DFT -> LDS at j*R + r.  The loads go through buffer
// descriptors built from scalars (one VGPR offset per butterfly, the r*N/R step as a scalar offset, range-checked by the hardware).
// Per-thread indices are derived anew inside every pass: opaque copies of tid and N keep the compiler from hoisting the address
// arithmetic of every pass variant out of the window loop, where it was held live across the whole loop and spilled.
__device__ __forceinline__ void mr_opaque(int& tid, int& n) {
  asm volatile("" : "+v"(tid));
  asm volatile("" : "+s"(n));
}

template <int FMT, int R>
__device__ __forceinline__ void mr_first(const SpecParams& p, const char* fbase, int start, float2* lds, int n, int tid, int T) {
  constexpr int NB = MrNb<R>::value;
  mr_opaque(tid, n);
  constexpr int SB = fmt_bytes(FMT);
  const int m = n / R;
  const float tap_sc = tap_scale<FMT>(p);
  const auto irsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(fbase), 0, p.frame_len * SB, 0x00020000);
  const auto wrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.window), 0, n * 4, 0x00020000);
  float2 v[NB][R];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int j = tid + i * T;
    if (j < m) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float w = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(wrsrc, j * 4, r * m * 4, 0)) * tap_sc;
        float2 x;
        if constexpr (FMT == FMT_C64) {
          const u32x2 b = __builtin_amdgcn_raw_buffer_load_b64(irsrc, (start + j) * SB, r * m * SB, 0);
          const unsigned xr = b.x, xi = b.y;
          x = make_float2(__uint_as_float(xr), __uint_as_float(xi));
        } else if constexpr (FMT == FMT_S16) {
          x = unpack_signed<FMT>(__builtin_amdgcn_raw_buffer_load_b32(irsrc, (start + j) * SB, r * m * SB, 0));
        } else if constexpr (FMT == FMT_S8) {
          x = unpack_signed<FMT>(__builtin_amdgcn_raw_buffer_load_b16(irsrc, (start + j) * SB, r * m * SB, 0));
        } else {
          const unsigned short b = __builtin_amdgcn_raw_buffer_load_b16(irsrc, (start + j) * SB, r * m * SB, 0);
          x = make_float2((float)(b & 0xff) - p.u8_offset, (float)(b >> 8) - p.u8_offset);
        }
        v[i][r] = make_float2(x.x * w, x.y * w);
      }
      mr_dft<R>(v[i]);
    }
  }
  __syncthreads();     // every thread has read what the previous window's last pass (or the previous frame's finish) left
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int j = tid + i * T;
    if (j < m) {
#pragma unroll
      for (int r = 0; r < R; ++r) lds[j * R + r] = v[i][r];
    }
  }
  __syncthreads();
}

// A middle pass: LDS -> twiddles -> R-point DFT -> LDS.  j = tid + i*T is carried as (j / ns, j mod ns), stepped by the
// wave-uniform T / ns and T mod ns: one division per pass instead of one per butterfly.
template <int R>
__device__ __forceinline__ void mr_mid(float2* lds, const float2* tw, int n, int ns, int tid, int T) {
  constexpr int NB = MrNb<R>::value;
  mr_opaque(tid, n);
  const int m = n / R;
  const int tq = T / ns, tr = T - tq * ns;
  const auto trsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float2*>(tw), 0, (R - 1) * ns * 8, 0x00020000);
  float2 v[NB][R];
  int dst[NB];
  int q = tid / ns, k = tid - q * ns;
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int j = tid + i * T;
    if (j < m) {
      dst[i] = q * ns * R + k;
#pragma unroll
      for (int r = 0; r < R; ++r) v[i][r] = lds[j + r * m];
#pragma unroll
      for (int r = 1; r < R; ++r) {
        const u32x2 t = __builtin_amdgcn_raw_buffer_load_b64(trsrc, k * 8, (r - 1) * ns * 8, 0);
        const unsigned tx = t.x, ty = t.y;
        v[i][r] = cmul(v[i][r], make_float2(__uint_as_float(tx), __uint_as_float(ty)));
      }
      mr_dft<R>(v[i]);
    }
    q += tq;
    k += tr;
    if (k >= ns) { k -= ns; ++q; }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int j = tid + i * T;
    if (j < m) {
#pragma unroll
      for (int r = 0; r < R; ++r) lds[dst[i] + r * ns] = v[i][r];
    }
  }
  __syncthreads();
}

template <int FMT>
__device__ __forceinline__ void mr_first_any(int radix, const SpecParams& p, const char* fbase, int start, float2* lds, int n,
                                             int tid, int T) {
  if (radix == 5) mr_first<FMT, 5>(p, fbase, start, lds, n, tid, T);
  else if (radix == 3) mr_first<FMT, 3>(p, fbase, start, lds, n, tid, T);
  else if (radix == 4) mr_first<FMT, 4>(p, fbase, start, lds, n, tid, T);
  else mr_first<FMT, 2>(p, fbase, start, lds, n, tid, T);
}

__device__ __forceinline__ void mr_mid_any(int radix, float2* lds, const float2* tw, int n, int ns, int tid, int T) {
  if (radix == 5) mr_mid<5>(lds, tw, n, ns, tid, T);
  else if (radix == 3) mr_mid<3>(lds, tw, n, ns, tid, T);
  else if (radix == 4) mr_mid<4>(lds, tw, n, ns, tid, T);
  else mr_mid<2>(lds, tw, n, ns, tid, T);
}

template <int FMT>
__global__ __launch_bounds__(MR_MAX_THREADS) void mixed_radix_kernel(const SpecParams p, const MrPlan plan) {
  constexpr int CM = 0;          // the AVG / MAX / MIN fold, decided at run time (p.cumu)
#include "ksa_mr_body.inc"
}

// The Welch PSD fold as a compile-time constant: a kernel of its own name, so that one mixed_radix_kernel per sample format
// stays the whole run-time-fold family.  (Included text and not a shared __device__ function on purpose: called through one,
// mixed_radix_kernel itself compiled to a different instruction stream.)
template <int FMT>
__global__ __launch_bounds__(MR_MAX_THREADS) void mixed_radix_psd_kernel(const SpecParams p, const MrPlan plan) {
  constexpr int CM = CUMU_PSD;
#include "ksa_mr_body.inc"
}

// The int8 / int16 forms (FMT_S8, FMT_S16) of both, again under a name of their own: mixed_radix_kernel / mixed_radix_psd_kernel stay
// one kernel per format of the complex64 / uint8 pair.  CMX = 0 (the run-time fold) or CUMU_PSD.
template <int FMT, int CMX>
__global__ __launch_bounds__(MR_MAX_THREADS) void mixed_radix_fixed_kernel(const SpecParams p, const MrPlan plan) {
  static_assert(FMT == FMT_S8 || FMT == FMT_S16, "signed fixed-point formats only");
  constexpr int CM = CMX;
#include "ksa_mr_body.inc"
}

}  // namespace ksa
