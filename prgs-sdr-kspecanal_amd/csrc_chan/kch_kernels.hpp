// libksa_chan: the polyphase channelizer of include/ksa_chan.h for gfx950.
//
// Both forms of the header run one kernel on a "virtual" input: hist_len unpacked samples (the stream's history, none in the
// block form) followed by the call's raw samples.  Column j of a block needs virt[off + j*D .. off + j*D + T); x[m*D - k] of the
// header is virt[off + j*D + (T-1) - k].  One workgroup owns W consecutive columns of one block, all M channels; it has 256, 512 or
// 1024 threads, the more the fewer workgroups its LDS lets a CU hold, so that a CU always has 16 waves to hide latency with (the
// host's plan).  Work items are independent, so the thread count moves no bit:
//
//   load     the tile's span, (W-1) D + T samples, into LDS once: 16-byte loads where a whole vector lies inside the input,
//            single samples at the edges, unpacking on the way in; the twiddle table (M/2 values) beside it.
//   branch   work item (w, p): u_w[p] = sum_q h[p + M q] * span[w D + (T-1) - p - M q], one chain of fused multiply-adds per
//            part, q ascending.  Lanes take consecutive p, so they read consecutive LDS words and consecutive taps (h itself is
//            the table: tap (p, q) is h[q M + p]).  u goes to the column's row of the workspace at the bit-reversed p.
//   fft      the radix-2 decimation-in-time network in place, two stages per pass (four points per work item, one barrier per
//            pass), after one single stage when log2 M is odd.  A column's row has pitch M + 1, so that the store phase, which
//            walks the columns, is free of bank conflicts.
//   store    work item (c, w): z_w[c] times (-i)^(c m 4/O) by swaps and signs, to out[(b M + c) chan_stride + m0 + w]: every
//            channel's W columns are one run of 8 W bytes.
//
// Chain order and network are functions of (M, O, P) alone; W only decides which columns share a workgroup.  Every arithmetic
// step of the unpack is spelled with an explicit rounding intrinsic, so that the history kernel and the loader give the same
// bits for the same sample.  All LDS is dynamic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../csrc_shared/ksa_iq.hpp"

namespace ksa {
namespace chan {

using iq::FMT_C64; using iq::FMT_U8; using iq::FMT_S8; using iq::FMT_S16;
using iq::Fmt; using iq::sample_of; using iq::sample_at;          // csrc_shared/ksa_iq.hpp: raw I,Q to float2
constexpr int MAX_THREADS = 1024;

struct Args {
  const void* iq;                   // raw samples of the call (block 0)
  const float2* hist;               // hist_len unpacked samples that precede them (stream form)
  const float* taps;                // [T]
  const float2* tw;                 // [max(M / 2, 1)]: exp(+2 pi i k / M)
  float2* out;                      // block b, channel c, column j at out[(b * M + c) * chan_stride + j]
  long long block_stride;           // samples
  long long chan_stride;
  int raw_len;                      // raw samples per block
  int hist_len;                     // T - 1 in the stream form, 0 in the block form
  int off;                          // virtual index of the oldest sample of column 0
  int ncol;                         // columns per block
  int tiles;                        // workgroups per block
  int m_first;                      // the stream's index of column 0, mod 4
  int W, logW;                      // columns per workgroup
  int M, logM, D, T, P;
  int rot;                          // 4 / O: quarter turns per unit of c * m
  int pitch;                        // float2 per column row of the workspace
  float u8_offset, u8_inv_scale;
};

// virtual samples [u0, u0 + span) of block `base` -> dst[0 .. span), unpacked; past the input: zero
template <int FMT>
__device__ __forceinline__ void load_span(const Args& a, const char* base, int u0, int span, float2* dst) {
  constexpr int B = Fmt<FMT>::BYTES, V = Fmt<FMT>::PER_VEC;
  const int tid = threadIdx.x, threads = blockDim.x;
  const int nh = min(span, max(0, a.hist_len - u0));            // leading samples that come from the history
  for (int s = tid; s < nh; s += threads) dst[s] = a.hist[u0 + s];
  const int nraw = span - nh;
  if (nraw <= 0) return;
  const int r0 = u0 + nh - a.hist_len;                          // first raw sample of the span
  const char* p0 = base + (size_t)r0 * B;
  const int mis = (int)((reinterpret_cast<uintptr_t>(p0) & 15u) / B);
  const char* v0 = p0 - (size_t)mis * B;                        // 16-byte aligned
  const int nvec = (nraw + mis + V - 1) / V;
  const int have = a.raw_len - r0;                              // raw samples from r0 to the end of the block
  for (int g = tid; g < nvec; g += threads) {
    const int j0 = g * V - mis;
    if (j0 >= 0 && j0 + V <= nraw && j0 + V <= have) {
      const uint4 w = *reinterpret_cast<const uint4*>(v0 + (size_t)g * 16);
#pragma unroll
      for (int e = 0; e < V; ++e) dst[nh + j0 + e] = sample_of<FMT>(w, e, a);
    } else {
      for (int e = 0; e < V; ++e) {
        const int j = j0 + e;
        if (j < 0 || j >= nraw) continue;
        float2 v = make_float2(0.f, 0.f);
        if (j < have) v = sample_at<FMT>(base, r0 + j, a);
        dst[nh + j] = v;
      }
    }
  }
}

__device__ __forceinline__ const char* block_base(const Args& a, int b, int bytes) {
  return static_cast<const char*>(a.iq) + (size_t)((long long)b * a.block_stride) * (size_t)bytes;
}

// w * b: each part one multiply and one fused multiply-add
__device__ __forceinline__ float2 cmul(float2 w, float2 b) {
  return make_float2(fmaf(w.x, b.x, -__fmul_rn(w.y, b.y)), fmaf(w.x, b.y, __fmul_rn(w.y, b.x)));
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y)); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(__fsub_rn(a.x, b.x), __fsub_rn(a.y, b.y)); }

template <int FMT>
__global__ __launch_bounds__(MAX_THREADS) void chan_kernel(const Args a) {
  extern __shared__ __attribute__((aligned(16))) float2 kch_lds[];
  const int M = a.M, logM = a.logM, W = a.W;
  float2* tw = kch_lds;                                            // [max(M / 2, 2)]
  float2* work = tw + max(M >> 1, 2);                              // [W * pitch], rounded up to even
  float2* span = work + ((W * a.pitch + 1) & ~1);                  // [(W - 1) D + T]
  const int tid = threadIdx.x, threads = blockDim.x;
  const int b = blockIdx.x / a.tiles, tile = blockIdx.x - b * a.tiles;
  const int m0 = tile * W;
  const int cnt = min(W, a.ncol - m0);

  for (int k = tid; k < max(M >> 1, 1); k += threads) tw[k] = a.tw[k];
  load_span<FMT>(a, block_base(a, b, Fmt<FMT>::BYTES), a.off + m0 * a.D, (cnt - 1) * a.D + a.T, span);
  __syncthreads();

  // branch sums.  The workgroup has at least M threads (a power of two, like M), so a thread keeps its p: it takes its columns
  // four at a time, one tap load serves all four, and four chains are in flight.  Each chain is still q ascending.
  {
    const int p = tid & (M - 1), total = cnt << logM;
    const float* h = a.taps + p;
    const float2* x0 = span + ((a.T - 1) - p);
    const int slot = (int)(__brev((unsigned)p) >> (32 - logM));
    for (int i0 = tid; i0 < total; i0 += 4 * threads) {
      const float2* x[4];
      float re[4], im[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = min(i0 + u * threads, total - 1);             // past the end: a valid column again, not stored
        x[u] = x0 + (i >> logM) * a.D;
        re[u] = im[u] = 0.f;
      }
#pragma unroll 2
      for (int q = 0; q < a.P; ++q) {
        const float t = h[q << logM];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float2 v = x[u][-(q << logM)];
          re[u] = fmaf(t, v.x, re[u]);
          im[u] = fmaf(t, v.y, im[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * threads;
        if (i < total) work[(i >> logM) * a.pitch + slot] = make_float2(re[u], im[u]);
      }
    }
  }
  __syncthreads();

  // the transform: stage of half-span hs pairs (i, i + hs), i mod 2 hs = j < hs, with tw[j * M / (2 hs)]
  int lh = 0;                                                      // log2 of the next stage's half-span
  if (logM & 1) {                                                  // one stage alone: its twiddle is (1, 0)
    for (int i = tid; i < (cnt << (logM - 1)); i += threads) {
      const int w = i >> (logM - 1), t = i & ((M >> 1) - 1);
      float2* e = work + w * a.pitch + 2 * t;
      const float2 x0 = e[0], x1 = e[1];
      e[0] = cadd(x0, x1);
      e[1] = csub(x0, x1);
    }
    __syncthreads();
    lh = 1;
  }
  for (; lh < logM; lh += 2) {                                     // stages hs and 2 hs in one pass
    const int hs = 1 << lh;
    for (int i = tid; i < (cnt << (logM - 2)); i += threads) {
      const int w = i >> (logM - 2), t = i & ((M >> 2) - 1);
      const int j = t & (hs - 1);
      float2* e = work + w * a.pitch + (((t >> lh) << (lh + 2)) + j);
      const float2 w1 = tw[j << (logM - 1 - lh)];
      const float2 w2 = tw[j << (logM - 2 - lh)];
      const float2 w3 = tw[(j + hs) << (logM - 2 - lh)];
      const float2 x0 = e[0], x1 = e[hs], x2 = e[2 * hs], x3 = e[3 * hs];
      const float2 t1 = cmul(w1, x1), t3 = cmul(w1, x3);
      const float2 a0 = cadd(x0, t1), a1 = csub(x0, t1), a2 = cadd(x2, t3), a3 = csub(x2, t3);
      const float2 s2 = cmul(w2, a2), s3 = cmul(w3, a3);
      e[0] = cadd(a0, s2);
      e[2 * hs] = csub(a0, s2);
      e[hs] = cadd(a1, s3);
      e[3 * hs] = csub(a1, s3);
    }
    __syncthreads();
  }

  // store: y[c][m] = z_m[c] * (-i)^(c m rot)
  float2* out = a.out + ((long long)b * M) * a.chan_stride + m0;
  for (int i = tid; i < (M << a.logW); i += threads) {
    const int w = i & (W - 1), c = i >> a.logW;
    if (w >= cnt) continue;
    const float2 z = work[w * a.pitch + c];
    const int k = (c * ((a.m_first + m0 + w) & 3) * a.rot) & 3;
    const float2 r = (k & 1) ? make_float2(z.y, -z.x) : z;         // times (0, -1)
    out[(long long)c * a.chan_stride + w] = (k & 2) ? make_float2(-r.x, -r.y) : r;
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
    dst[i] = sample_at<FMT>(static_cast<const char*>(a.iq), u - a.hist_len, a);
  }
}

// power[c] = sum over the channel's rows (row r * M + c, r < nrows) of |buf[row * stride + first + j]|^2, j < count, in float64:
// thread t takes j = t, t + 256, .. of every row, rows in order; the 256 partial sums meet in a fixed tree
__global__ __launch_bounds__(256) void power_kernel(const float2* buf, long long stride, int M, int nrows, long long first, int count,
                                                    double* power) {
  extern __shared__ __attribute__((aligned(16))) double kch_red[];
  const int c = blockIdx.x, tid = threadIdx.x;
  double acc = 0.0;
  for (int r = 0; r < nrows; ++r) {
    const float2* row = buf + ((long long)r * M + c) * stride + first;
    for (int j = tid; j < count; j += 256) {
      const float2 v = row[j];
      const double re = (double)v.x, im = (double)v.y;
      acc = __dadd_rn(acc, __dadd_rn(__dmul_rn(re, re), __dmul_rn(im, im)));
    }
  }
  kch_red[tid] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) kch_red[tid] = __dadd_rn(kch_red[tid], kch_red[tid + s]);
    __syncthreads();
  }
  if (tid == 0) power[c] = kch_red[0];
}

}  // namespace chan
}  // namespace ksa
