// Kernels of libksa_density (include/ksa_density.h): the density histogram's add pass and its element-wise companions.
//
// add_kernel<VEC, COMBINE>: one workgroup takes a strip of S bitmap columns (S*g adjacent bins) x all L+1 levels for a chunk of
// input rows.  Its partial histogram lives in LDS as uint32 [L+1][pitch] and takes ds_add_u32; the chunk is short enough that
// rows * g < 2^32, so a cell cannot wrap.  After the chunk the non-zero cells go to the global int64 counters by integer
// atomicAdd (exact, order-free).  Lanes walk ADJACENT bins of a row; where the strip is narrower than a wave the next lanes take
// the next row.  pitch = S | 1 is odd: lanes that share a column (other rows, or g > 1) but differ in level then differ in LDS
// bank too.  VEC: 16-byte loads (row base, stride and strip start all 16-byte aligned), else one float per lane.  COMBINE
// (g > 1): runs of adjacent lanes with the same cell are added once, by the run's first lane with the run length -- a constant
// row costs one atomic per wave instead of 64 on one address.
#pragma once
#include <hip/hip_runtime.h>

namespace ksa {
namespace density {

constexpr int THREADS = 256;
constexpr int ROWS_UNROLL = 4;      // independent row loads in flight per lane

struct AddArgs {
  const float* rows;
  long long row_stride;             // floats
  unsigned long long* counts;       // [L + 1][W]
  int nrows, W, g, L, S, pitch, nstrips, chunk_rows;
  float lo, inv;
};

// include/ksa_density.h, "Semantics": one subtraction, one multiplication.  Branch-free form of its four cases: max(t, 0) takes
// t < 0 (and -inf) to level 0, min(., L - 0.5) takes t >= L (and +inf) to level L - 1 -- L - 0.5 is exact for L <= 1024 and
// truncates to L - 1 like every t in [L - 1, L) --, truncation does the rest.  A NaN never reaches the conversion (fmaxf
// returns its other operand) and is sent to the extra row by the test on x itself.
__device__ __forceinline__ unsigned level_of(float x, float lo, float inv, unsigned L, float top) {
  const float t = __fmul_rn(__fsub_rn(x, lo), inv);
  const unsigned row = (unsigned)(int)fminf(fmaxf(t, 0.0f), top);
  return x != x ? L : row;
}

template <bool COMBINE>
__device__ __forceinline__ void hit(unsigned* lds, bool valid, unsigned cell, int lane) {
  if (COMBINE) {
    const unsigned key = valid ? cell : 0x80000000u + (unsigned)lane;      // idle lanes never join a run
    const unsigned prev = __shfl_up(key, 1);
    const bool head = lane == 0 || key != prev;
    const unsigned long long heads = __ballot(head);
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    const unsigned run = above ? (unsigned)__ffsll((long long)above) : (unsigned)(64 - lane);
    if (head && valid) atomicAdd(&lds[cell], run);
  } else {
    if (valid) atomicAdd(&lds[cell], 1u);
  }
}

// ROWS_UNROLL rows of one lane: rows u * rpp apart from p, all loaded before the first is counted.  FULL: every one of them
// exists (left > 0 for all); else row u exists when u * rpp < left.
template <bool VEC, bool COMBINE, bool FULL>
__device__ __forceinline__ void rows_pass(unsigned* lds, const AddArgs& a, const float* p, long long step, int rpp, bool qok, int left,
                                          const unsigned (&col)[VEC ? 4 : 1], int lane, float top) {
  constexpr int E = VEC ? 4 : 1;
  float x[ROWS_UNROLL][E];
  bool ok[ROWS_UNROLL];
#pragma unroll
  for (int u = 0; u < ROWS_UNROLL; ++u) {
    ok[u] = qok && (FULL || u * rpp < left);
#pragma unroll
    for (int j = 0; j < E; ++j) x[u][j] = 0.0f;
    if (ok[u]) {
      if constexpr (VEC) {
        const float4 v = *reinterpret_cast<const float4*>(p + u * step);
        x[u][0] = v.x; x[u][1] = v.y; x[u][2] = v.z; x[u][3] = v.w;
      } else {
        x[u][0] = p[u * step];
      }
    }
  }
#pragma unroll
  for (int u = 0; u < ROWS_UNROLL; ++u) {
#pragma unroll
    for (int j = 0; j < E; ++j) {
      const unsigned cell = level_of(x[u][j], a.lo, a.inv, (unsigned)a.L, top) * (unsigned)a.pitch + col[j];
      hit<COMBINE>(lds, ok[u], cell, lane);
    }
  }
}

template <bool VEC, bool COMBINE>
__global__ __launch_bounds__(THREADS) void add_kernel(const AddArgs a) {
  extern __shared__ unsigned lds[];
  constexpr int E = VEC ? 4 : 1;
  const int tid = threadIdx.x, lane = tid & 63;
  const int strip = blockIdx.x % a.nstrips, chunk = blockIdx.x / a.nstrips;
  const int col0 = strip * a.S;
  const int ncols = min(a.S, a.W - col0);
  const int nbe = ncols * a.g / E;                      // elements (floats or float4) of a row that this strip holds
  const long long row0 = (long long)chunk * a.chunk_rows;
  const int nr = (int)min((long long)a.chunk_rows, (long long)a.nrows - row0);
  const int cells = (a.L + 1) * a.pitch;
  for (int i = tid; i < cells; i += THREADS) lds[i] = 0;
  __syncthreads();

  // lanes-per-row: a power of two so that a lane keeps its bins (and their columns) for every row
  int lpr = 1;
  while (lpr < nbe && lpr < THREADS) lpr <<= 1;
  const int rpp = THREADS / lpr;                        // rows per pass of the workgroup
  const int q0 = tid & (lpr - 1), rr = tid / lpr;
  const float top = (float)a.L - 0.5f;
  const float* base = a.rows + row0 * a.row_stride + (long long)col0 * a.g;

  for (int qb = 0; qb < nbe; qb += lpr) {               // trip counts are workgroup-uniform: COMBINE's shuffles see whole waves
    const int q = qb + q0;
    const bool qok = q < nbe;
    unsigned col[E];
#pragma unroll
    for (int j = 0; j < E; ++j) col[j] = qok ? (unsigned)((q * E + j) / a.g) : 0u;
    const float* p = base + (long long)(qok ? q : 0) * E + (long long)rr * a.row_stride;
    const long long step = (long long)rpp * a.row_stride;
    int rb = 0;
    for (; rb + rpp * ROWS_UNROLL <= nr; rb += rpp * ROWS_UNROLL, p += step * ROWS_UNROLL)      // every row of the pass exists
      rows_pass<VEC, COMBINE, true>(lds, a, p, step, rpp, qok, nr, col, lane, top);
    for (; rb < nr; rb += rpp * ROWS_UNROLL, p += step * ROWS_UNROLL)
      rows_pass<VEC, COMBINE, false>(lds, a, p, step, rpp, qok, nr - rb - rr, col, lane, top);
  }
  __syncthreads();

  const int out = (a.L + 1) * ncols;
  for (int i = tid; i < out; i += THREADS) {
    const int lvl = i / ncols, c = i - lvl * ncols;
    const unsigned v = lds[lvl * a.pitch + c];
    if (v) atomicAdd(&a.counts[(long long)lvl * a.W + col0 + c], (unsigned long long)v);
  }
}

// floor(c * num / den) without a product that leaves 64 bits (c >= 0, 0 <= num <= den < 2^31)
__global__ void decay_kernel(long long* counts, long long n, long long num, long long den) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const long long c = counts[i];
    counts[i] = (c / den) * num + ((c % den) * num) / den;
  }
}

__global__ void merge_kernel(long long* counts, const long long* other, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    counts[i] += other[i];
}

__global__ void reset_kernel(long long* counts, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    counts[i] = 0;
}

}  // namespace density
}  // namespace ksa
