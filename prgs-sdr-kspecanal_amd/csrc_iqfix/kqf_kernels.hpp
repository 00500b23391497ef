// libksa_iqfix: the DC-offset and IQ-imbalance corrector of include/ksa_iqfix.h for gfx950.
//
// One memory-bound pass, fix_kernel<FMT, APPLY, ACC>: the apply-only, the accumulate-only and the combined form are the same
// kernel with the other half compiled out.  A tile is TILE = 4096 consecutive samples of one block, 256 threads; a workgroup
// takes the tiles w, w + grid, ... of the call, so that the partial sums have a fixed size whatever the call.
//
// Loads: 16 bytes per lane (iq::Fmt<FMT>::PER_VEC samples) where a vector lies wholly inside the tile, single samples at its
// ends (a scalar head up to the first 16-byte boundary and a scalar tail).  Stores: the PER_VEC outputs of a lane are 8 PER_VEC
// contiguous bytes; they leave as 16-byte stores, with one 8-byte store at either end when the output is 8 bytes off the
// 16-byte grid.  A sample is read and written by the same thread, which is what lets complex64 run in place.
//
// Sums: each of the five integers of a sample is an integer-valued float r, |r| <= 2^32, split exactly into
// r = 65536 hi + lo, 0 <= lo < 65536, by a floor and a fused multiply-add whose result is exact; hi and lo go through the 32-bit
// conversion and into int32 sums that a thread keeps for one tile (at most TILE / THREADS + PER_VEC samples: below 2^21 each),
// and which it folds into its five int64 accumulators at the tile's end.  The accumulators are reduced in the wave with lane
// swaps, across the waves through LDS, and each workgroup leaves one record of five int64.  finish_kernel (one workgroup)
// adds the records to the object's sums: the stream orders it behind the pass and in front of the next, so that no two
// workgroups ever update one word.
// Integer sums are associative, so neither tile nor grid nor the cut into calls can enter the result.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../csrc_shared/ksa_iq.hpp"

namespace ksa {
namespace iqfix {

constexpr int THREADS = 256;
constexpr int TILE = 4096;                          // samples a workgroup takes at a time
constexpr int MAX_GRID = 4096;                      // workgroups of a launch, and records of partial sums
constexpr int NSUMS = 5;                            // aI, aQ, cII, cQQ, cIQ; word 5 of the object's sums is the count
constexpr float UNIT = 1073741824.0f;               // 2^30

struct Args {
  const void* in;                   // the call's raw samples (block 0)
  float2* out;                      // block b, sample i at [b out_stride + i]; not read without APPLY
  long long* partials;              // [grid][NSUMS]; not read without ACC
  long long block_stride;           // samples
  long long out_stride;             // samples
  long long ntiles;                 // tiles of the launch
  float u8_offset, u8_inv_scale;
  float dc_i, dc_q, c, d;           // by value: a launch keeps the coefficients it was enqueued with
  int len;                          // samples per block
  int tiles;                        // tiles per block
};

// One rounding per operation: a product formed here carries no licence to be contracted into a fused multiply-add with the
// sum it feeds.
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float sub_rn(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}

__device__ __forceinline__ float2 corrected(const Args& a, const float2 x) {
  const float ui = sub_rn(x.x, a.dc_i), uq = sub_rn(x.y, a.dc_q);
  return make_float2(ui, add_rn(mul_rn(a.c, ui), mul_rn(a.d, uq)));
}

// the int32 sums of one thread over one tile
struct TileSums {
  int hi[NSUMS], lo[NSUMS];
};

// v is clamped to [-4, 4]: rintf(v 2^30) as 65536 hi + lo, every step exact
__device__ __forceinline__ void add_quantity(TileSums& s, int k, float v) {
  const float r = rintf(mul_rn(v, UNIT));
  const float h = floorf(mul_rn(r, 0.0000152587890625f));       // 2^-16: |h| <= 2^16
  const float l = fmaf(h, -65536.0f, r);                        // 0 .. 65535, exact
  s.hi[k] += (int)h;
  s.lo[k] += (int)l;
}

__device__ __forceinline__ float clamp4(float v) { return fmaxf(fminf(v, 4.0f), -4.0f); }

__device__ __forceinline__ void add_sample(TileSums& s, const float2 x) {
  add_quantity(s, 0, clamp4(x.x));
  add_quantity(s, 1, clamp4(x.y));
  add_quantity(s, 2, fminf(mul_rn(x.x, x.x), 4.0f));
  add_quantity(s, 3, fminf(mul_rn(x.y, x.y), 4.0f));
  add_quantity(s, 4, clamp4(mul_rn(x.x, x.y)));
}

// y[0 .. V) to q, which is aligned to 8 bytes
template <int V> __device__ __forceinline__ void store_outputs(float2* q, const float2 (&y)[V]) {
  if ((reinterpret_cast<uintptr_t>(q) & 15u) == 0) {
#pragma unroll
    for (int e = 0; e < V; e += 2) *reinterpret_cast<float4*>(q + e) = make_float4(y[e].x, y[e].y, y[e + 1].x, y[e + 1].y);
  } else {
    q[0] = y[0];
    asm volatile("" ::: "memory");                              // keeps the two forms apart: merged, neither is a 16-byte store
#pragma unroll
    for (int e = 1; e + 1 < V; e += 2) *reinterpret_cast<float4*>(q + e) = make_float4(y[e].x, y[e].y, y[e + 1].x, y[e + 1].y);
    q[V - 1] = y[V - 1];
  }
}

// v[NSUMS] summed over the workgroup; the result is valid in thread 0
__device__ __forceinline__ void block_sum(long long (&v)[NSUMS]) {
  __shared__ long long wave_sum[THREADS / 64][NSUMS];
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < NSUMS; ++k)
    for (int m = 32; m; m >>= 1) v[k] += __shfl_xor(v[k], m);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NSUMS; ++k) wave_sum[tid >> 6][k] = v[k];
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < NSUMS; ++k) {
      long long t = 0;
      for (int w = 0; w < THREADS / 64; ++w) t += wave_sum[w][k];
      v[k] = t;
    }
  }
}

template <int FMT, bool APPLY, bool ACC> __global__ __launch_bounds__(THREADS) void fix_kernel(const Args a) {
  constexpr int V = iq::Fmt<FMT>::PER_VEC, BYTES = iq::Fmt<FMT>::BYTES;
  const int tid = threadIdx.x;
  long long acc[NSUMS] = {0, 0, 0, 0, 0};
  for (long long w = blockIdx.x; w < a.ntiles; w += gridDim.x) {
    const long long b = w / a.tiles;
    const int i0 = (int)(w - b * a.tiles) * TILE;
    const int count = min(TILE, a.len - i0);
    const char* base = static_cast<const char*>(a.in) + (size_t)(b * a.block_stride) * BYTES;
    const char* p0 = base + (size_t)i0 * BYTES;
    const int mis = (int)((reinterpret_cast<uintptr_t>(p0) & 15u) / BYTES);
    const char* v0 = p0 - mis * BYTES;                          // 16-byte aligned; only read where a whole vector is inside
    const int nvec = (count + mis + V - 1) / V;
    float2* ob = APPLY ? a.out + (b * a.out_stride + i0) : nullptr;
    TileSums s = {};
    for (int g = tid; g < nvec; g += THREADS) {
      const int j0 = V * g - mis;
      if (j0 >= 0 && j0 + V <= count) {
        const uint4 wv = *reinterpret_cast<const uint4*>(v0 + (size_t)g * 16);
        float2 y[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float2 x = iq::sample_of<FMT>(wv, e, a);
          if (ACC) add_sample(s, x);
          if (APPLY) y[e] = corrected(a, x);
        }
        if (APPLY) store_outputs<V>(ob + j0, y);
      } else {
        for (int e = 0; e < V; ++e) {
          const int j = j0 + e;
          if (j >= 0 && j < count) {
            const float2 x = iq::sample_at<FMT>(base, i0 + j, a);
            if (ACC) add_sample(s, x);
            if (APPLY) ob[j] = corrected(a, x);
          }
        }
      }
    }
    if (ACC) {
#pragma unroll
      for (int k = 0; k < NSUMS; ++k) acc[k] += (long long)s.hi[k] * 65536ll + (long long)s.lo[k];
    }
  }
  if (ACC) {
    block_sum(acc);
    if (tid == 0) {
#pragma unroll
      for (int k = 0; k < NSUMS; ++k) a.partials[(long long)blockIdx.x * NSUMS + k] = acc[k];
    }
  }
}

// the records of a pass of `grid` workgroups over `count` samples into the object's six words
__global__ __launch_bounds__(THREADS) void finish_kernel(const long long* partials, int grid, long long count, long long* sums) {
  long long v[NSUMS] = {0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < grid; i += THREADS) {
#pragma unroll
    for (int k = 0; k < NSUMS; ++k) v[k] += partials[(long long)i * NSUMS + k];
  }
  block_sum(v);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < NSUMS; ++k) sums[k] += v[k];
    sums[NSUMS] += count;
  }
}

}  // namespace iqfix
}  // namespace ksa
