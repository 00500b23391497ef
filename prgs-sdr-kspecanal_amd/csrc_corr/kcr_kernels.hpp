// libksa_corr: the matched-filter correlator and peak list of include/ksa_corr.h for gfx950.
//
// Both forms of the header run the same kernels on a "virtual" input: hist_len unpacked samples from the stream's history (none
// in the block form) followed by the call's raw samples.
//
// corr_kernel<Q>.  One workgroup of 256 threads owns a tile of W = 256 R consecutive lags (R = 8 for Q <= 2, 4 above: W and R
// are a function of Q alone, the LDS bytes of (K, Q)) and brings the tile's span of W + K - 1 samples into LDS once, unpacked to
// complex64, with 16-byte loads where a vector lies wholly inside the block and single samples elsewhere; what lies past the
// span is zero.  Thread t holds the R consecutive lags t R .. t R + R-1 and slides a window of R samples in registers over the
// span: per tap k it reads ONE new sample from LDS and the Q template values c_q[k], which are the same for every lane, and
// spends (4 Q + 2) R fused multiply-adds.  k is unrolled by R, so the window rotates by register renaming.  The accumulator of
// a (lag, template) is the register pair (re, im): the two terms of a tap are two packed fused multiply-adds,
// (re, im) += (xr, xr) * (cr, -ci) and (re, im) += (xi, xi) * (ci, cr), each half the fmaf the header writes; the host lays
// the table out as those two pairs per tap.  The energy chain stays two plain fused multiply-adds per lag and tap.
//
// LDS layout: sample s of the span lies at row s mod R, column s div R.  At tap k = a R + b the thread needs sample
// t R + k + R, which is row b, column t + a + 1: the 64 lanes of a wave read 64 consecutive complex values, no bank is hit
// twice, whatever R is.
//
// The template values arrive by scalar loads from the table in device memory (the constant address space: the address is a
// function of the kernel's arguments and the loop counter alone).  They cost neither LDS bandwidth nor vector registers, a
// packed fused multiply-add takes a pair of them as its scalar operand, and the table (at most 256 KiB, read in step by every
// wave) stays in the scalar cache and the L2.  An LDS broadcast would spend one more LDS read per k and template on a kernel whose other
// limit, after the fp32 pipes, is LDS.
//
// Every chain is ordered by k alone: re and im of each (lag, template) and the window energy e of each lag start at +0 and take
// their two terms per k in the order the header fixes.  Neither the tile nor the grid nor the cut of a stream enters.  A
// workgroup walks tiles blockIdx.x, blockIdx.x + gridDim.x, ...: the grid is capped, the tile count is not.
//
// The kernel leaves rho and r of every lag of the launch in the object's work buffers, row (block, template), and, where the
// caller asked, in the dense outputs.  pick_kernel reads them: an item is one (block, lag, template) in exactly the order of the
// event list, a workgroup owns a chunk of 1024 consecutive items.  pick_kernel<false> counts the peaks of every chunk,
// sum_kernel / offset_kernel turn the counts into the place of every chunk's first record behind the records the list already
// holds, and pick_kernel<true> repeats the chunks that have a peak and stores each record at its place: whatever order the
// workgroups run in, the list is in ascending (block, pos, templ) order, and no atomic is involved.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../csrc_shared/ksa_iq.hpp"

namespace ksa {
namespace corr {

constexpr int THREADS = 256;
constexpr int CHUNK_PER_THREAD = 4;
constexpr int CHUNK = THREADS * CHUNK_PER_THREAD;   // items per workgroup of the peak stage
constexpr int SCAN_THREADS = 256;                   // chunks per workgroup of the offset scan
constexpr int EVENT_WORDS = 9;                      // kcr_event: 36 bytes, no padding

__host__ __device__ constexpr int lags_per_thread(int Q) { return Q <= 2 ? 8 : 4; }
__host__ __device__ constexpr int round_up(int K, int R) { return (K + R - 1) / R * R; }
// columns of one LDS row: 256 window starts, the K taps beyond them, one more so that the last prefetch stays inside
__host__ __device__ constexpr int row_len(int K, int R) { return THREADS + round_up(K, R) / R + 1; }

struct Args {
  const void* in;                   // the call's raw samples (block 0)
  const float2* hist;               // hist_len unpacked samples that precede them (stream form)
  const float* tmpl;                // [Q][K][4]: (cr, -ci, ci, cr), what the two packed multiply-adds of a tap take
  const float* ec;                  // [Q] template energies
  float* rho;                       // work: block b, template q, lag i at [(b Q + q) nl + i]
  float2* r;                        // work, the same layout
  float* metric_out;                // dense rho or null: [(b Q + q) out_stride + i - dense_first]
  float2* corr_out;                 // dense r or null
  long long block_stride;           // samples
  long long out_stride;             // values
  long long tiles;                  // tiles per block
  long long total;                  // tiles of the launch
  int fmt;
  float u8_offset, u8_inv_scale;
  int raw_len;                      // samples per block
  int hist_len;
  int v0;                           // virtual index of the sample that meets c[0] at work lag 0
  int nl;                           // lags per block
  int dense_first;                  // work lag of the first dense value
  int K;
  float min_energy;
};

template <int R> __device__ __forceinline__ int lds_pos(int s, int row) { return (s & (R - 1)) * row + (s / R); }

// virtual samples [u0, u0 + span) of the block at base -> dst[lds_pos(0 .. span)], zero from span to fill
template <int FMT, int R>
__device__ __forceinline__ void load_span(const Args& a, const char* base, int u0, int span, int fill, int row, float2* dst) {
  constexpr int V = iq::Fmt<FMT>::PER_VEC, BYTES = iq::Fmt<FMT>::BYTES;
  const int tid = threadIdx.x;
  const int nh = min(span, max(0, a.hist_len - u0));            // leading samples that come from the history
  for (int s = tid; s < nh; s += THREADS) dst[lds_pos<R>(s, row)] = a.hist[u0 + s];
  for (int s = span + tid; s < fill; s += THREADS) dst[lds_pos<R>(s, row)] = make_float2(0.f, 0.f);
  const int nraw = span - nh;
  if (nraw <= 0) return;
  const int r0 = u0 + nh - a.hist_len;                          // first sample of the block that the span needs
  const char* p0 = base + (size_t)r0 * BYTES;
  const int mis = (int)((reinterpret_cast<uintptr_t>(p0) & 15u) / BYTES);
  const char* v0 = p0 - mis * BYTES;                            // 16-byte aligned; only read where a whole vector is inside
  const int nvec = (nraw + mis + V - 1) / V;
  const int have = a.raw_len - r0;                              // samples from r0 to the end of the block
  for (int g = tid; g < nvec; g += THREADS) {
    const int j0 = V * g - mis;
    if (j0 >= 0 && j0 + V <= nraw && j0 + V <= have) {
      const uint4 w = *reinterpret_cast<const uint4*>(v0 + (size_t)g * 16);
#pragma unroll
      for (int e = 0; e < V; ++e) dst[lds_pos<R>(nh + j0 + e, row)] = iq::sample_of<FMT>(w, e, a);
    } else {
      for (int e = 0; e < V; ++e) {
        const int j = j0 + e;
        if (j < 0 || j >= nraw) continue;
        dst[lds_pos<R>(nh + j, row)] = j < have ? iq::sample_at<FMT>(base, r0 + j, a) : make_float2(0.f, 0.f);
      }
    }
  }
}

typedef const __attribute__((address_space(4))) float* uniform_floats;   // loads through it are scalar loads

typedef float float_pair __attribute__((ext_vector_type(2)));

// z = (re, im): one packed fused multiply-add serves both parts, each lane of it an fmaf of its own
template <int Q, int R> struct Acc {
  float_pair z[R][Q];
  float e[R];
};

// taps k0 .. k0 + R-1 (those below K when !FULL); win holds samples t R + k0 .. t R + k0 + R-1, sample t R + m in slot m mod R
template <int Q, int R, bool FULL>
__device__ __forceinline__ void taps_block(Acc<Q, R>& acc, float_pair (&win)[R], const float_pair* lds, int row, int col,
                                           uniform_floats c, int K, int k0) {
  float_pair nxt[R];
#pragma unroll
  for (int b = 0; b < R; ++b) nxt[b] = lds[b * row + col];     // the R reads are in flight together
#pragma unroll
  for (int b = 0; b < R; ++b) {
    if (FULL || k0 + b < K) {
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int t = 4 * (q * K + k0 + b);
        const float_pair by_xr = {c[t], c[t + 1]}, by_xi = {c[t + 2], c[t + 3]};     // (cr, -ci), (ci, cr)
#pragma unroll
        for (int j = 0; j < R; ++j) {
          const float_pair x = win[(b + j) % R];
          acc.z[j][q] = __builtin_elementwise_fma(x.xx, by_xr, acc.z[j][q]);     // re += xr cr,  im += xr (-ci)
          acc.z[j][q] = __builtin_elementwise_fma(x.yy, by_xi, acc.z[j][q]);     // re += xi ci,  im += xi cr
        }
      }
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const float_pair x = win[(b + j) % R];
        acc.e[j] = fmaf(x.x, x.x, acc.e[j]);
        acc.e[j] = fmaf(x.y, x.y, acc.e[j]);
      }
      win[b] = nxt[b];
    }
  }
}

template <int Q>
__global__ __launch_bounds__(THREADS) void corr_kernel(const Args a) {
  constexpr int R = lags_per_thread(Q), W = THREADS * R;
  extern __shared__ __attribute__((aligned(16))) float2 kcr_lds[];
  const int K = a.K, row = row_len(K, R), fill = W + round_up(K, R);
  const int tid = threadIdx.x;
  const int bytes = a.fmt == iq::FMT_C64 ? 8 : a.fmt == iq::FMT_S16 ? 4 : 2;
  const uniform_floats c = reinterpret_cast<uniform_floats>(reinterpret_cast<uintptr_t>(a.tmpl));
  const uniform_floats ec = reinterpret_cast<uniform_floats>(reinterpret_cast<uintptr_t>(a.ec));
  for (long long w = blockIdx.x; w < a.total; w += gridDim.x) {
    const long long b = w / a.tiles;
    const int i0 = (int)((w - b * a.tiles) * W);                // the tile's first lag of its block
    const int cnt = min(W, a.nl - i0);
    const int span = cnt + K - 1;
    const char* base = static_cast<const char*>(a.in) + (size_t)(b * a.block_stride) * bytes;
    switch (a.fmt) {
      case iq::FMT_C64: load_span<iq::FMT_C64, R>(a, base, a.v0 + i0, span, fill, row, kcr_lds); break;
      case iq::FMT_U8: load_span<iq::FMT_U8, R>(a, base, a.v0 + i0, span, fill, row, kcr_lds); break;
      case iq::FMT_S8: load_span<iq::FMT_S8, R>(a, base, a.v0 + i0, span, fill, row, kcr_lds); break;
      default: load_span<iq::FMT_S16, R>(a, base, a.v0 + i0, span, fill, row, kcr_lds); break;
    }
    __syncthreads();

    Acc<Q, R> acc;
    const float_pair* span_lds = reinterpret_cast<const float_pair*>(kcr_lds);
    float_pair win[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
      win[j] = span_lds[j * row + tid];
      acc.e[j] = 0.f;
#pragma unroll
      for (int q = 0; q < Q; ++q) acc.z[j][q] = float_pair{0.f, 0.f};
    }
    int k = 0, col = tid + 1;
    for (; k + R <= K; k += R, ++col) taps_block<Q, R, true>(acc, win, span_lds, row, col, c, K, k);
    if (k < K) taps_block<Q, R, false>(acc, win, span_lds, row, col, c, K, k);

#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int i = tid * R + j;
      if (i >= cnt) continue;
      const int lag = i0 + i;
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const float re = acc.z[j][q].x, im = acc.z[j][q].y;
        const float p = fmaf(re, re, __fmul_rn(im, im));
        const float den = __fmul_rn(acc.e[j], ec[q]);
        const float rho = (den > 0.f && acc.e[j] >= a.min_energy) ? __fdiv_rn(p, den) : 0.f;
        const long long rowq = b * Q + q;
        a.rho[rowq * a.nl + lag] = rho;
        a.r[rowq * a.nl + lag] = make_float2(re, im);
        if (lag >= a.dense_first) {
          const long long o = rowq * a.out_stride + (lag - a.dense_first);
          if (a.metric_out) a.metric_out[o] = rho;
          if (a.corr_out) a.corr_out[o] = make_float2(re, im);
        }
      }
    }
    __syncthreads();                                            // the next tile's loads overwrite the span
  }
}

// the stream's new history after a call of raw_len samples: dst[i] = virt[i + shift], i < keep (dst is not a.hist)
__global__ __launch_bounds__(THREADS) void history_kernel(const Args a, float2* dst, int keep, int shift) {
  const int i = blockIdx.x * THREADS + threadIdx.x;
  if (i >= keep) return;
  const int u = i + shift;
  float2 v;
  if (u < a.hist_len) {
    v = a.hist[u];
  } else {
    const char* base = static_cast<const char*>(a.in);
    const int r = u - a.hist_len;
    switch (a.fmt) {
      case iq::FMT_C64: v = iq::sample_at<iq::FMT_C64>(base, r, a); break;
      case iq::FMT_U8: v = iq::sample_at<iq::FMT_U8>(base, r, a); break;
      case iq::FMT_S8: v = iq::sample_at<iq::FMT_S8>(base, r, a); break;
      default: v = iq::sample_at<iq::FMT_S16>(base, r, a); break;
    }
  }
  dst[i] = v;
}

struct PickArgs {
  const float* rho;                 // work, [(b Q + q) nl + i]
  const float2* r;
  int* cnt;                         // [chunks] peaks per chunk: written by the counting pass, read by the emitting pass
  const long long* off;             // [chunks] place of the chunk's first record (emitting pass)
  unsigned* events;                 // [capacity][EVENT_WORDS]
  long long items;                  // nblocks * nd * Q
  long long pos_base;               // position of work lag 0
  int stream;                       // 1: block is -1
  int nl;                           // lags per row; the lags outside [0, nl) do not exist
  int d_a, nd;                      // the lags decided: work lags [d_a, d_a + nd)
  int Q, G, capacity;
  float threshold;
};

template <bool EMIT>
__global__ __launch_bounds__(THREADS) void pick_kernel(const PickArgs a) {
  __shared__ int wave_sum[THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if constexpr (EMIT) {
    if (a.cnt[blockIdx.x] == 0) return;                         // workgroup-uniform
  }
  const long long first = (long long)blockIdx.x * CHUNK + (long long)tid * CHUNK_PER_THREAD;
  bool peak[CHUNK_PER_THREAD];
  int mine = 0;
#pragma unroll
  for (int u = 0; u < CHUNK_PER_THREAD; ++u) {
    const long long item = first + u;
    peak[u] = false;
    if (item >= a.items) continue;
    const long long t = item / a.Q;
    const int q = (int)(item - t * a.Q);
    const long long b = t / a.nd;
    const int i = a.d_a + (int)(t - b * a.nd);
    const float* row = a.rho + (b * a.Q + q) * a.nl;
    const float v = row[i];
    if (!(v >= a.threshold)) continue;
    bool ok = true;
    const int lo = max(i - a.G, 0), hi = min(i + a.G, a.nl - 1);
    for (int j = i + 1; ok && j <= hi; ++j) ok = !(row[j] > v);
    for (int j = i - 1; ok && j >= lo; --j) ok = !(row[j] >= v);
    peak[u] = ok;
    mine += ok ? 1 : 0;
  }
  int inc = mine;                                               // inclusive over the wave
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  if (lane == 63) wave_sum[wave] = inc;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) {
    if (w < wave) before += wave_sum[w];
    all += wave_sum[w];
  }
  if constexpr (!EMIT) {
    if (tid == 0) a.cnt[blockIdx.x] = all;
  } else {
    long long place = a.off[blockIdx.x] + before + inc - mine;
#pragma unroll
    for (int u = 0; u < CHUNK_PER_THREAD; ++u) {
      if (!peak[u]) continue;
      if (place < (long long)a.capacity) {
        const long long item = first + u;
        const long long t = item / a.Q;
        const int q = (int)(item - t * a.Q);
        const long long b = t / a.nd;
        const int i = a.d_a + (int)(t - b * a.nd);
        const long long at = (b * a.Q + q) * a.nl + i;
        const long long pos = a.pos_base + i;
        const float2 r = a.r[at];
        unsigned* e = a.events + place * EVENT_WORDS;
        e[0] = (unsigned)((unsigned long long)pos & 0xffffffffull);
        e[1] = (unsigned)((unsigned long long)pos >> 32);
        e[2] = a.stream ? 0xffffffffu : (unsigned)b;
        e[3] = (unsigned)q;
        e[4] = __float_as_uint(a.rho[at]);
        e[5] = __float_as_uint(i > 0 ? a.rho[at - 1] : 0.f);
        e[6] = __float_as_uint(i + 1 < a.nl ? a.rho[at + 1] : 0.f);
        e[7] = __float_as_uint(r.x);
        e[8] = __float_as_uint(r.y);
      }
      ++place;
    }
  }
}

struct ScanArgs {
  const int* cnt;                   // [n]
  int n;                            // chunks
  long long* block_sums;            // [ceil(n / SCAN_THREADS)]
  long long* total;                 // events_total
  long long* snapshot;              // events_total as it was before this launch
  long long* off;                   // [n]
};

__global__ __launch_bounds__(SCAN_THREADS) void sum_kernel(const ScanArgs a) {
  __shared__ long long part[SCAN_THREADS / 64];
  const int tid = threadIdx.x, i = blockIdx.x * SCAN_THREADS + tid;
  long long s = i < a.n ? a.cnt[i] : 0;
  for (int m = 32; m; m >>= 1) s += __shfl_xor(s, m);
  if ((tid & 63) == 0) part[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    long long all = 0;
    for (int w = 0; w < SCAN_THREADS / 64; ++w) all += part[w];
    a.block_sums[blockIdx.x] = all;
    if (blockIdx.x == 0) *a.snapshot = *a.total;
  }
}

__global__ __launch_bounds__(SCAN_THREADS) void offset_kernel(const ScanArgs a) {
  constexpr int SW = SCAN_THREADS / 64;
  __shared__ long long before[SW];
  __shared__ int wave_sum[SW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long part = 0;
  for (int b = tid; b < (int)blockIdx.x; b += SCAN_THREADS) part += a.block_sums[b];
  for (int m = 32; m; m >>= 1) part += __shfl_xor(part, m);
  const int i = blockIdx.x * SCAN_THREADS + tid;
  const int c = i < a.n ? a.cnt[i] : 0;
  int inc = c;                                                  // at most 256 chunks of at most 1024 peaks
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(inc, d);
    if (lane >= d) inc += t;
  }
  if (lane == 0) before[wave] = part;
  if (lane == 63) wave_sum[wave] = inc;
  __syncthreads();
  long long pos = *a.snapshot;
  int mine = inc - c, all = 0;
#pragma unroll
  for (int w = 0; w < SW; ++w) {
    pos += before[w];
    if (w < wave) mine += wave_sum[w];
    all += wave_sum[w];
  }
  if (i < a.n) a.off[i] = pos + mine;
  if (blockIdx.x == gridDim.x - 1 && tid == 0) *a.total = pos + all;
}

}  // namespace corr
}  // namespace ksa
