// libksa_demod: the detector and the decimating real FIR of include/ksa_demod.h for gfx950.
//
// Both forms of the header run one kernel on a "virtual" input of demodulated real samples: hist_len of them from the stream's
// history (none in the block form) followed by the detector's values of the call's raw samples.  Output j of a block is
// sum_k h[k] * virt[off + j*D + (T-1) - k].  One workgroup of 256 threads owns a tile of consecutive outputs and brings the
// tile's span of (tile - 1) * D + T demodulated samples into LDS once: the history part is copied, the raw part is read with
// 16-byte loads (two complex64 samples) from the 16-byte boundary at or below the first needed sample, single samples where a
// vector does not lie wholly inside the call's input, and the detector runs on the way in; FM reads the one sample in front
// of a vector as well.  The filter then only reads LDS.
//
// The span lies in LDS as D phase rows (sample s at [s % D][s / D], the row pitch odd), so that the 64 lanes of a wave, which
// hold consecutive outputs and hence samples D apart, read consecutive floats.  Row and column of a tap are wave-uniform; the
// taps come through scalar loads.  A thread holds R outputs 256 apart (tile = 256 R), or the first `tile` threads hold one
// each where the span of 256 does not fit.  Every output is one chain of fused multiply-adds over k = 0 .. T-1: its order is
// a function of k alone, and the tile is a function of D and T, so results do not depend on tile, grid or how a stream is cut.
// Every arithmetic step of the detector is spelled out in detect(), the one function that both loader paths and the history
// kernel call, so that the same sample gives the same bits everywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ksa {
namespace demod {

constexpr int MODE_AM = 0, MODE_FM = 1, MODE_PM = 2;
constexpr int THREADS = 256;
constexpr int LDS_MAX = (63 * 256 + 4096 + 2 * 256) * 4;   // the largest span of any plan with its padding: every tile kernel's limit

struct Args {
  const float2* iq;                 // raw samples of the call (block 0)
  const float* hist;                // hist_len demodulated samples that precede them (stream form)
  const float2* last;               // the raw sample in front of raw sample 0 (stream form), else null: zero
  const float* taps;                // [T]
  void* out;                        // block b, output m at out[b * out_stride + m], float or short
  long long block_stride;           // samples
  long long out_stride;
  int raw_len;                      // raw samples per block
  int hist_len;                     // T - 1 in the stream form, 0 in the block form
  int off;                          // virtual index of the oldest sample of output 0: < D (stream), lead (block)
  int nout;                         // outputs per block
  int tiles;                        // workgroups per block
  int tile_out;                     // outputs per workgroup
  int D, T;
  unsigned magic;                   // ceil(2^32 / D) for D > 1: s / D = umulhi(s, magic) while s * D < 2^32
  int pitch;                        // floats per phase row
  float pcm_scale;
};

// atan2f(im, re) / 2 pi in [-0.5, 0.5], exact on the axes: include/ksa_demod.h, "Detector"
__device__ __forceinline__ float turns(float re, float im) {
  float t = __fmul_rn(atan2f(im, re), 0.15915494309189535f);
  t = fminf(fmaxf(t, -0.5f), 0.5f);
  if (im == 0.f) t = re < 0.f ? 0.5f : 0.f;
  else if (re == 0.f) t = im > 0.f ? 0.25f : -0.25f;
  return t;
}

// d[n] of x = x[n] and y = x[n-1] (FM only).  sqrtf is the correctly rounded one (the compiler's default for HIP).
template <int MODE> __device__ __forceinline__ float detect(float2 x, float2 y) {
  if (MODE == MODE_AM) return sqrtf(fmaf(x.x, x.x, __fmul_rn(x.y, x.y)));
  if (MODE == MODE_PM) return turns(x.x, x.y);
  const float pr = fmaf(x.x, y.x, __fmul_rn(x.y, y.y));
  const float pi = fmaf(x.y, y.x, -__fmul_rn(x.x, y.y));
  return turns(pr, pi);
}

// the raw sample in front of raw sample r >= 0 of the block at base
__device__ __forceinline__ float2 sample_before(const Args& a, const float2* base, int r) {
  if (r > 0) return base[r - 1];
  return a.last ? *a.last : make_float2(0.f, 0.f);
}

// d of raw sample r of the block at base
template <int MODE> __device__ __forceinline__ float detect_at(const Args& a, const float2* base, int r) {
  return detect<MODE>(base[r], MODE == MODE_FM ? sample_before(a, base, r) : make_float2(0.f, 0.f));
}

__device__ __forceinline__ int lds_pos(int s, const Args& a) {
  const int q = a.D == 1 ? s : (int)__umulhi((unsigned)s, a.magic);
  return (s - q * a.D) * a.pitch + q;
}

// virtual samples [u0, u0 + span) of block `base` -> dst[lds_pos(0 .. span)], demodulated; past the input: zero
template <int MODE>
__device__ __forceinline__ void load_span(const Args& a, const float2* base, int u0, int span, float* dst) {
  const int tid = threadIdx.x;
  const int nh = min(span, max(0, a.hist_len - u0));            // leading samples that come from the history
  for (int s = tid; s < nh; s += THREADS) dst[lds_pos(s, a)] = a.hist[u0 + s];
  const int nraw = span - nh;
  if (nraw <= 0) return;
  const int r0 = u0 + nh - a.hist_len;                          // first raw sample of the span
  const float2* p0 = base + r0;
  const int mis = (int)((reinterpret_cast<uintptr_t>(p0) & 15u) >> 3);
  const float2* v0 = p0 - mis;                                  // 16-byte aligned
  const int nvec = (nraw + mis + 1) >> 1;
  const int have = a.raw_len - r0;                              // raw samples from r0 to the end of the block
  for (int g = tid; g < nvec; g += THREADS) {
    const int j0 = 2 * g - mis;
    if (j0 >= 0 && j0 + 2 <= nraw && j0 + 2 <= have) {
      const float4 w = *reinterpret_cast<const float4*>(v0 + 2 * g);
      const float2 x0 = make_float2(w.x, w.y), x1 = make_float2(w.z, w.w);
      const float2 y0 = MODE == MODE_FM ? sample_before(a, base, r0 + j0) : make_float2(0.f, 0.f);
      dst[lds_pos(nh + j0, a)] = detect<MODE>(x0, y0);
      dst[lds_pos(nh + j0 + 1, a)] = detect<MODE>(x1, x0);
    } else {
      for (int e = 0; e < 2; ++e) {
        const int j = j0 + e;
        if (j < 0 || j >= nraw) continue;
        dst[lds_pos(nh + j, a)] = j < have ? detect_at<MODE>(a, base, r0 + j) : 0.f;
      }
    }
  }
}

__device__ __forceinline__ void store(float* out, int m, float y, float) { out[m] = y; }
__device__ __forceinline__ void store(short* out, int m, float y, float pcm_scale) {
  const float p = __fmul_rn(y, pcm_scale);      // NaN is tested here: fmaxf(NaN, c) is c, the clamp would hide it
  const float v = p != p ? 0.f : fminf(fmaxf(rintf(p), -32768.f), 32767.f);
  out[m] = (short)(int)v;
}

template <int MODE, int R, typename OUT>
__global__ __launch_bounds__(THREADS) void tile_kernel(const Args a) {
  extern __shared__ __attribute__((aligned(16))) float kdm_lds[];
  const int b = blockIdx.x / a.tiles, tile = blockIdx.x - b * a.tiles;
  const int m0 = tile * a.tile_out;
  const int cnt = min(a.tile_out, a.nout - m0);
  load_span<MODE>(a, a.iq + (size_t)((long long)b * a.block_stride), a.off + m0 * a.D, (cnt - 1) * a.D + a.T, kdm_lds);
  __syncthreads();
  if ((int)threadIdx.x >= a.tile_out) return;     // a tile below 256 outputs: whole waves leave (no barrier follows)
  float acc[R];
#pragma unroll
  for (int j = 0; j < R; ++j) acc[j] = 0.f;
  // tap k meets sample m*D + e, e = T-1-k, of output m: phase row e % D, column m + e / D
  int col = (a.T - 1) / a.D, row = (a.T - 1) - col * a.D;
  const float* mine = kdm_lds + threadIdx.x;
  int k = 0;
  for (; k + 4 <= a.T; k += 4) {       // four taps at a time: their loads are in flight together; the sum keeps its order
    float h[4];
    const float* p[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      h[u] = a.taps[k + u];
      p[u] = mine + row * a.pitch + col;
      if (--row < 0) { row = a.D - 1; --col; }
    }
    float v[4][R];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < R; ++j) v[u][j] = p[u][j * THREADS];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < R; ++j) acc[j] = fmaf(h[u], v[u][j], acc[j]);
  }
  for (; k < a.T; ++k) {
    const float h = a.taps[k];
    const float* p = mine + row * a.pitch + col;
#pragma unroll
    for (int j = 0; j < R; ++j) acc[j] = fmaf(h, p[j * THREADS], acc[j]);
    if (--row < 0) { row = a.D - 1; --col; }
  }
  OUT* out = static_cast<OUT*>(a.out) + (long long)b * a.out_stride + m0;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const int m = threadIdx.x + j * THREADS;
    if (m < cnt) store(out, m, acc[j], a.pcm_scale);
  }
}

// the stream's new state after a call of raw_len samples: dst_hist[i] = virt[i + raw_len], i < T-1, and the last raw sample
// (dst_hist is not a.hist, dst_last is not a.last)
template <int MODE>
__global__ __launch_bounds__(THREADS) void history_kernel(const Args a, float* dst_hist, float2* dst_last) {
  const int i = blockIdx.x * THREADS + threadIdx.x;
  if (i == 0) *dst_last = a.iq[a.raw_len - 1];
  if (i >= a.T - 1) return;
  const int u = i + a.raw_len;
  dst_hist[i] = u < a.hist_len ? a.hist[u] : detect_at<MODE>(a, a.iq, u - a.hist_len);
}

}  // namespace demod
}  // namespace ksa
