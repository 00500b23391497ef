// libksa_ddc: the mixing, decimating FIR of include/ksa_ddc.h for gfx950.
//
// Both forms of the header run one kernel on a "virtual" input: hist_len already mixed samples (the stream's history, none in
// the block form) followed by the call's raw samples.  Output j of a block is sum_k h[k] * virt[off + j*D + (T-1) - k].  One
// workgroup owns a tile of consecutive outputs, brings the tile's span into LDS once (16-byte loads where a whole vector lies
// inside the input, single samples at the edges), unpacking and mixing every sample on the way in, and then only reads LDS.
//
//   tile_kernel    256 threads, R outputs per thread (tile = 256 R).  The span lies in LDS as D phase rows (sample s at
//                  [s % D][s / D], the row pitch odd), so that the 64 lanes of a wave, which hold consecutive outputs and hence
//                  samples D apart, read consecutive addresses.  Row and column of a tap are wave-uniform; the taps come through
//                  scalar loads.  Every output is one chain of fused multiply-adds over k = 0 .. T-1.
//   reduce_kernel  512 threads, 8 outputs per workgroup, for spans that do not fit: the span is walked in chunks of 8192
//                  samples, the taps lie in LDS, thread i owns the taps k = i (mod 512) of every output, highest k first, and
//                  the 512 partial sums meet in a fixed tree (xor shuffles 32 .. 1, then the 8 waves in order).
//
// The order of an output's sum is a function of k alone in either form, and the form is a function of D and T: results do not
// depend on tile, grid or how a stream is cut.  Every arithmetic step of unpack and mixer is spelled with an explicit rounding
// intrinsic, so that the history kernel and both loaders give the same bits for the same sample.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../csrc_shared/ksa_iq.hpp"

namespace ksa {
namespace ddc {

using iq::FMT_C64; using iq::FMT_U8; using iq::FMT_S8; using iq::FMT_S16;
using iq::Fmt; using iq::sample_of; using iq::sample_at;          // csrc_shared/ksa_iq.hpp: raw I,Q to float2
constexpr int TILE_THREADS = 256;
constexpr int RED_THREADS = 512;
constexpr int RED_WAVES = RED_THREADS / 64;
constexpr int RED_OUT = 8;          // outputs per workgroup of the reduce form
constexpr int RED_CHUNK = 8192;     // samples of the span in LDS at a time

struct Args {
  const void* iq;                   // raw samples of the call (block 0)
  const float2* hist;               // hist_len mixed samples that precede them (stream form)
  const float* taps;                // [T]
  float2* out;                      // block b, output m at out[b * out_stride + m]
  long long block_stride;           // samples
  long long out_stride;
  unsigned long long phase0;        // phase of raw sample 0 of every block
  unsigned long long phase_inc;
  int raw_len;                      // raw samples per block
  int hist_len;                     // T - 1 in the stream form, 0 in the block form
  int off;                          // virtual index of the oldest sample of output 0, < D
  int nout;                         // outputs per block
  int tiles;                        // workgroups per block
  int tile_out;                     // outputs per workgroup
  int D, T;
  unsigned magic;                   // ceil(2^32 / D) for D > 1: s / D = umulhi(s, magic) while s * D < 2^32
  int pitch;                        // tile form: float2 per phase row
  float u8_offset, u8_inv_scale;
};

// x * (cos 2 pi phi, -sin 2 pi phi), phi in 2^-64 turns: include/ksa_ddc.h, "Mixer"
__device__ __forceinline__ float2 mix(float2 x, unsigned long long phi) {
  const unsigned r = (unsigned)(phi >> 32) + 0x20000000u;       // nearest quarter turn and what is left of it
  const unsigned q = r >> 30;
  const int f = (int)(r & 0x3fffffffu) - 0x20000000;            // [-2^29, 2^29) in 2^-32 turns
  const float th = __fmul_rn((float)f, 1.4629180792671596e-9f); // 2 pi 2^-32
  const float z = __fmul_rn(th, th);
  float s = fmaf(z, -1.9515295891e-4f, 8.3321608736e-3f);
  s = fmaf(z, s, -1.6666654611e-1f);
  s = fmaf(__fmul_rn(z, th), s, th);
  float c = fmaf(z, 2.443315711809948e-5f, -1.388731625493765e-3f);
  c = fmaf(z, c, 4.166664568298827e-2f);
  c = fmaf(__fmul_rn(z, z), c, fmaf(z, -0.5f, 1.0f));
  float2 y;                                                     // x * (c, -s)
  y.x = fmaf(x.x, c, __fmul_rn(x.y, s));
  y.y = fmaf(x.y, c, -__fmul_rn(x.x, s));
  if (f == 0) y = x;
  const float2 t = (q & 1u) ? make_float2(y.y, -y.x) : y;       // times (0, -1)
  return (q & 2u) ? make_float2(-t.x, -t.y) : t;                // times (-1, 0)
}

template <bool POLY> __device__ __forceinline__ int lds_pos(int s, const Args& a) {
  if (!POLY) return s;
  const int q = a.D == 1 ? s : (int)__umulhi((unsigned)s, a.magic);
  return (s - q * a.D) * a.pitch + q;
}

// virtual samples [u0, u0 + span) of block `base` -> dst[lds_pos(0 .. span)], unpacked and mixed; past the input: zero
template <int FMT, bool POLY, int THREADS>
__device__ __forceinline__ void load_span(const Args& a, const char* base, int u0, int span, float2* dst) {
  constexpr int B = Fmt<FMT>::BYTES, V = Fmt<FMT>::PER_VEC;
  const int tid = threadIdx.x;
  const int nh = min(span, max(0, a.hist_len - u0));            // leading samples that come from the history
  for (int s = tid; s < nh; s += THREADS) dst[lds_pos<POLY>(s, a)] = a.hist[u0 + s];
  const int nraw = span - nh;
  if (nraw <= 0) return;
  const int r0 = u0 + nh - a.hist_len;                          // first raw sample of the span
  const char* p0 = base + (size_t)r0 * B;
  const int mis = (int)((reinterpret_cast<uintptr_t>(p0) & 15u) / B);
  const char* v0 = p0 - (size_t)mis * B;                        // 16-byte aligned
  const int nvec = (nraw + mis + V - 1) / V;
  const int have = a.raw_len - r0;                              // raw samples from r0 to the end of the block
  for (int g = tid; g < nvec; g += THREADS) {
    const int j0 = g * V - mis;
    if (j0 >= 0 && j0 + V <= nraw && j0 + V <= have) {
      const uint4 w = *reinterpret_cast<const uint4*>(v0 + (size_t)g * 16);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const int j = j0 + e;
        dst[lds_pos<POLY>(nh + j, a)] = mix(sample_of<FMT>(w, e, a), a.phase0 + (unsigned long long)(unsigned)(r0 + j) * a.phase_inc);
      }
    } else {
      for (int e = 0; e < V; ++e) {
        const int j = j0 + e;
        if (j < 0 || j >= nraw) continue;
        float2 v = make_float2(0.f, 0.f);
        if (j < have) v = mix(sample_at<FMT>(base, r0 + j, a), a.phase0 + (unsigned long long)(unsigned)(r0 + j) * a.phase_inc);
        dst[lds_pos<POLY>(nh + j, a)] = v;
      }
    }
  }
}

__device__ __forceinline__ const char* block_base(const Args& a, int b, int bytes) {
  return static_cast<const char*>(a.iq) + (size_t)((long long)b * a.block_stride) * (size_t)bytes;
}

template <int FMT, int R>
__global__ __launch_bounds__(TILE_THREADS) void tile_kernel(const Args a) {
  extern __shared__ float2 kdc_lds[];
  const int b = blockIdx.x / a.tiles, tile = blockIdx.x - b * a.tiles;
  const int m0 = tile * a.tile_out;
  const int cnt = min(a.tile_out, a.nout - m0);
  load_span<FMT, true, TILE_THREADS>(a, block_base(a, b, Fmt<FMT>::BYTES), a.off + m0 * a.D, (cnt - 1) * a.D + a.T, kdc_lds);
  __syncthreads();
  float2 acc[R];
#pragma unroll
  for (int j = 0; j < R; ++j) acc[j] = make_float2(0.f, 0.f);
  // tap k meets sample m*D + e, e = T-1-k, of output m: phase row e % D, column m + e / D
  int col = (a.T - 1) / a.D, row = (a.T - 1) - col * a.D;
  const float2* mine = kdc_lds + threadIdx.x;
  int k = 0;
  for (; k + 4 <= a.T; k += 4) {       // four taps at a time: their loads are in flight together; the sum keeps its order
    float h[4];
    const float2* p[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      h[u] = a.taps[k + u];
      p[u] = mine + row * a.pitch + col;
      if (--row < 0) { row = a.D - 1; --col; }
    }
    float2 v[4][R];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < R; ++j) v[u][j] = p[u][j * TILE_THREADS];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < R; ++j) {
        acc[j].x = fmaf(h[u], v[u][j].x, acc[j].x);
        acc[j].y = fmaf(h[u], v[u][j].y, acc[j].y);
      }
  }
  for (; k < a.T; ++k) {
    const float h = a.taps[k];
    const float2* p = mine + row * a.pitch + col;
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const float2 v = p[j * TILE_THREADS];
      acc[j].x = fmaf(h, v.x, acc[j].x);
      acc[j].y = fmaf(h, v.y, acc[j].y);
    }
    if (--row < 0) { row = a.D - 1; --col; }
  }
  float2* out = a.out + (long long)b * a.out_stride + m0;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const int m = threadIdx.x + j * TILE_THREADS;
    if (m < cnt) out[m] = acc[j];
  }
}

template <int FMT>
__global__ __launch_bounds__(RED_THREADS) void reduce_kernel(const Args a) {
  extern __shared__ float2 kdc_lds[];
  float2* smp = kdc_lds;                                           // [RED_CHUNK]
  float2* red = kdc_lds + RED_CHUNK;                               // [RED_WAVES][RED_OUT]
  float* taps = reinterpret_cast<float*>(red + RED_WAVES * RED_OUT);  // [T]
  const int tid = threadIdx.x;
  const int b = blockIdx.x / a.tiles, tile = blockIdx.x - b * a.tiles;
  const int m0 = tile * RED_OUT;
  const int cnt = min(RED_OUT, a.nout - m0);
  const int u0 = a.off + m0 * a.D, span = (cnt - 1) * a.D + a.T;
  const char* base = block_base(a, b, Fmt<FMT>::BYTES);
  for (int k = tid; k < a.T; k += RED_THREADS) taps[k] = a.taps[k];
  float2 acc[RED_OUT];
#pragma unroll
  for (int j = 0; j < RED_OUT; ++j) acc[j] = make_float2(0.f, 0.f);
  for (int c0 = 0; c0 < span; c0 += RED_CHUNK) {
    const int c1 = min(span, c0 + RED_CHUNK);
    __syncthreads();                                               // the chunk before is consumed (first pass: nothing)
    load_span<FMT, false, RED_THREADS>(a, base, u0 + c0, c1 - c0, smp);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RED_OUT; ++j) {
      if (j >= cnt) continue;
      const int top = j * a.D + a.T - 1;                           // tap k meets sample top - k of the span
      const int kmax = min(a.T - 1, top - c0), kmin = max(0, top - c1 + 1);
      const int d = kmax - tid;
      if (d < 0) continue;
      for (int k = tid + (d & ~(RED_THREADS - 1)); k >= kmin; k -= RED_THREADS) {
        const float2 v = smp[top - k - c0];
        const float h = taps[k];
        acc[j].x = fmaf(h, v.x, acc[j].x);
        acc[j].y = fmaf(h, v.y, acc[j].y);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < RED_OUT; ++j) {
    float re = acc[j].x, im = acc[j].y;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      re = __fadd_rn(re, __shfl_xor(re, o));
      im = __fadd_rn(im, __shfl_xor(im, o));
    }
    if ((tid & 63) == 0) red[(tid >> 6) * RED_OUT + j] = make_float2(re, im);
  }
  __syncthreads();
  if (tid < cnt) {
    float2 s = red[tid];
    for (int w = 1; w < RED_WAVES; ++w) {
      s.x = __fadd_rn(s.x, red[w * RED_OUT + tid].x);
      s.y = __fadd_rn(s.y, red[w * RED_OUT + tid].y);
    }
    a.out[(long long)b * a.out_stride + m0 + tid] = s;
  }
}

// the stream's new history: dst[i] = virt[i + n_in], i < T-1 (dst is not a.hist)
template <int FMT>
__global__ __launch_bounds__(256) void history_kernel(const Args a, float2* dst) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.T - 1) return;
  const int u = i + a.raw_len;
  if (u < a.hist_len) {
    dst[i] = a.hist[u];
  } else {
    const int r = u - a.hist_len;
    dst[i] = mix(sample_at<FMT>(static_cast<const char*>(a.iq), r, a), a.phase0 + (unsigned long long)(unsigned)r * a.phase_inc);
  }
}

}  // namespace ddc
}  // namespace ksa
