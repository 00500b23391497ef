// libksa_resamp: the polyphase L / M resampler of include/ksa_resamp.h for gfx950.
//
// Both forms of the header run one kernel on a "virtual" input: hist_len raw samples from the stream's history (none in the
// block form) followed by the call's samples.  Output j of a call (or of a block) is output m = m_f + j of the definition; with
// t = m M, n = t div L and p = t mod L it reads the P virtual samples u .. u + P-1, u = n_f + (n(m) - n(m_f)), the oldest
// first, so that tap q meets virtual sample u + (P-1) - q.  The host hands over the position of output 0 alone, split into
// (n_f, p_f), and c_f = m_f mod L; a workgroup forms the position of its tile's first output from them in 64 bits (t leaves 32
// bits inside one permitted call: L = 1024 and 2^22 samples already reach 2^32), and its lanes add offsets of at most
// 1023 M + L - 1 < 2^25 to it.
//
// Neighbouring outputs use different tap sets: the phase walks by M mod L per output.  The taps therefore lie in device memory
// permuted by the host, g[q][i] = h[q L + (i M mod L)], so that output m reads g[q][m mod L] and the 64 lanes of a wave, which
// hold consecutive outputs, read consecutive floats of one row (wrapping at L); the table is at most 64 KiB and stays in the
// vector cache.  One workgroup of 256 threads owns a tile of W consecutive outputs and brings the tile's span of
// (W-1) M / L + P samples into LDS once, with 16-byte loads from the 16-byte boundary at or below the first needed sample and
// single samples where a vector does not lie wholly inside the call's input; the filter then reads samples from LDS only.
//
// LDS layout: sample s of the span lies at element s + (s >> 5), one element of padding after every 32.  Lanes are M / L
// samples apart: below one the lanes of a group read the same or neighbouring elements (broadcast, no conflict); at the
// power-of-two strides 2, 4, 8, 16 the padding turns what would be a 2- to 16-way conflict of ds_read_b32 (32 banks) or
// ds_read_b64 (64 banks) into a conflict-free access, since every 32 / stride lanes the bank moves on by one.
//
// A thread holds R outputs 256 apart (W = 256 R).  Every output is one chain of fused multiply-adds over q = 0 .. P-1 that
// starts at zero: its order is a function of q alone, and W is a function of (type, L, M, P), so results do not depend on tile,
// grid or how a stream is cut.  A workgroup walks tiles blockIdx.x, blockIdx.x + gridDim.x, ...: the grid is capped, the tile
// count is not.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ksa {
namespace resamp {

constexpr int THREADS = 256;
constexpr int LDS_FOUR = 40 * 1024;   // four workgroups per CU: one loads while the others filter

struct Args {
  const void* in;                   // the call's samples (block 0), float or float2
  const void* hist;                 // hist_len raw samples that precede them (stream form)
  const float* taps;                // g[P][L], the permuted table
  void* out;                        // block b, output j at out[b * out_stride + j]
  long long block_stride;           // samples
  long long out_stride;             // values
  long long nout;                   // outputs per block
  long long tiles;                  // tiles per block
  long long total;                  // tiles of the call
  long long c_f;                    // m_f mod L
  int raw_len;                      // samples per block
  int hist_len;                     // P - 1 in the stream form, 0 in the block form
  int n_f;                          // virtual index of the oldest sample of output 0
  int p_f;                          // phase of output 0
  int L, M, P;
  int tile_out;                     // W
  float pcm_scale;
};

__device__ __forceinline__ int lds_pos(int s) { return s + (s >> 5); }

__device__ __forceinline__ float zero_of(const float*) { return 0.f; }
__device__ __forceinline__ float2 zero_of(const float2*) { return make_float2(0.f, 0.f); }

__device__ __forceinline__ void put_vec(float* dst, int s, const float4& w) {
  dst[lds_pos(s)] = w.x; dst[lds_pos(s + 1)] = w.y; dst[lds_pos(s + 2)] = w.z; dst[lds_pos(s + 3)] = w.w;
}
__device__ __forceinline__ void put_vec(float2* dst, int s, const float4& w) {
  dst[lds_pos(s)] = make_float2(w.x, w.y); dst[lds_pos(s + 1)] = make_float2(w.z, w.w);
}

// virtual samples [u0, u0 + span) of the block at base -> dst[lds_pos(0 .. span)]; past the input: zero
template <typename E>
__device__ __forceinline__ void load_span(const Args& a, const E* base, int u0, int span, E* dst) {
  constexpr int V = 16 / (int)sizeof(E);                        // samples per 16-byte vector
  const int tid = threadIdx.x;
  const E* hist = static_cast<const E*>(a.hist);
  const int nh = min(span, max(0, a.hist_len - u0));            // leading samples that come from the history
  for (int s = tid; s < nh; s += THREADS) dst[lds_pos(s)] = hist[u0 + s];
  const int nraw = span - nh;
  if (nraw <= 0) return;
  const int r0 = u0 + nh - a.hist_len;                          // first sample of the call that the span needs
  const E* p0 = base + r0;
  const int mis = (int)((reinterpret_cast<uintptr_t>(p0) & 15u) / sizeof(E));
  const E* v0 = p0 - mis;                                       // 16-byte aligned; only read where a whole vector is inside
  const int nvec = (nraw + mis + V - 1) / V;
  const int have = a.raw_len - r0;                              // samples from r0 to the end of the block
  for (int g = tid; g < nvec; g += THREADS) {
    const int j0 = V * g - mis;
    if (j0 >= 0 && j0 + V <= nraw && j0 + V <= have) {
      put_vec(dst, nh + j0, *reinterpret_cast<const float4*>(v0 + V * g));
    } else {
      for (int e = 0; e < V; ++e) {
        const int j = j0 + e;
        if (j < 0 || j >= nraw) continue;
        dst[lds_pos(nh + j)] = j < have ? base[r0 + j] : zero_of(base);
      }
    }
  }
}

struct Acc1 { float v; };
struct Acc2 { float re, im; };
__device__ __forceinline__ void mac(Acc1& acc, float h, float x) { acc.v = fmaf(h, x, acc.v); }
__device__ __forceinline__ void mac(Acc2& acc, float h, float2 x) { acc.re = fmaf(h, x.x, acc.re); acc.im = fmaf(h, x.y, acc.im); }

__device__ __forceinline__ void store(float* out, long long m, const Acc1& y, float) { out[m] = y.v; }
__device__ __forceinline__ void store(float2* out, long long m, const Acc2& y, float) { out[m] = make_float2(y.re, y.im); }
__device__ __forceinline__ void store(short* out, long long m, const Acc1& y, float pcm_scale) {
  const float p = __fmul_rn(y.v, pcm_scale);    // NaN is tested here: fmaxf(NaN, c) is c, the clamp would hide it
  const float v = p != p ? 0.f : fminf(fmaxf(rintf(p), -32768.f), 32767.f);
  out[m] = (short)(int)v;
}

template <typename E> struct AccOf { typedef Acc1 type; };
template <> struct AccOf<float2> { typedef Acc2 type; };

// E: float or float2 samples; R outputs per thread; OUT: E, or short for int16 PCM of real samples
template <typename E, int R, typename OUT>
__global__ __launch_bounds__(THREADS) void tile_kernel(const Args a) {
  typedef typename AccOf<E>::type ACC;
  extern __shared__ __attribute__((aligned(16))) float krs_lds[];
  E* lds = reinterpret_cast<E*>(krs_lds);
  for (long long w = blockIdx.x; w < a.total; w += gridDim.x) {
    const long long b = w / a.tiles, tile = w - b * a.tiles;
    const long long m0 = tile * a.tile_out;                     // the tile's first output of its block
    const int cnt = (int)min((long long)a.tile_out, a.nout - m0);
    const long long t0 = a.p_f + m0 * a.M;                      // position of output m0 relative to n_f L, 64 bits
    const long long adv = t0 / a.L;                             // < raw_len
    const int p_t = (int)(t0 - adv * a.L);
    const int u0 = a.n_f + (int)adv;
    const int c_t = (int)((a.c_f + m0) % a.L);
    const int span = (int)(((unsigned)p_t + (unsigned)(cnt - 1) * (unsigned)a.M) / (unsigned)a.L) + a.P;
    const E* base = static_cast<const E*>(a.in) + (size_t)(b * a.block_stride);
    load_span<E>(a, base, u0, span, lds);
    __syncthreads();

    ACC acc[R];
    int s[R];                                                   // span index of the newest sample (tap 0)
    const float* g[R];                                          // tap 0 of this output's phase
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int i = min((int)threadIdx.x + j * THREADS, cnt - 1);   // a lane past the tile's end repeats the last output
      acc[j] = ACC{};
      s[j] = (int)(((unsigned)p_t + (unsigned)i * (unsigned)a.M) / (unsigned)a.L) + a.P - 1;
      g[j] = a.taps + (unsigned)(c_t + i) % (unsigned)a.L;
    }
    int q = 0;
    for (; q + 4 <= a.P; q += 4) {     // four taps at a time: their loads are in flight together; the sum keeps its order
      float h[4][R];
      E x[4][R];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < R; ++j) {
          h[u][j] = g[j][(q + u) * a.L];
          x[u][j] = lds[lds_pos(s[j] - q - u)];
        }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < R; ++j) mac(acc[j], h[u][j], x[u][j]);
    }
    for (; q < a.P; ++q) {
#pragma unroll
      for (int j = 0; j < R; ++j) mac(acc[j], g[j][q * a.L], lds[lds_pos(s[j] - q)]);
    }
    OUT* out = static_cast<OUT*>(a.out) + b * a.out_stride + m0;
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int i = threadIdx.x + j * THREADS;
      if (i < cnt) store(out, i, acc[j], a.pcm_scale);
    }
    __syncthreads();                                            // the next tile's loads overwrite the span
  }
}

// the stream's new history after a call of raw_len samples: dst[i] = virt[i + raw_len], i < P-1 (dst is not a.hist)
template <typename E>
__global__ __launch_bounds__(THREADS) void history_kernel(const Args a, E* dst) {
  const int i = blockIdx.x * THREADS + threadIdx.x;
  if (i >= a.P - 1) return;
  const int u = i + a.raw_len;
  dst[i] = u < a.hist_len ? static_cast<const E*>(a.hist)[u] : static_cast<const E*>(a.in)[u - a.hist_len];
}

}  // namespace resamp
}  // namespace ksa
