// Kernel of libksa_measure (include/ksa_measure.h): channel power, moments, peak, occupied bandwidth and x-dB width of windows
// of dB rows.
//
// measure_kernel<WG, VEC>: a TEAM measures one task (a row and a window [a, b]).  WG = false is the wave form: a team is one
// 64-lane wave, a workgroup of 256 threads holds four teams, every reduction and the prefix scan run across lanes by
// __shfl and there is no barrier and no LDS.  WG = true is the workgroup form: a team is the 256 threads, the waves' partial
// results meet in 208 bytes of LDS, two barriers per task.  The wave form takes the windows of at most WAVE_MAX_BINS bins
// (at most 4 bins, or two 16-byte loads, per lane), the workgroup form the wider ones; either kernel walks the whole task
// list by grid-stride and passes over the tasks of the other, so a list of mixed widths is two launches and no sorting.
//
// A task is read where it lies: span i of a list in device memory whose count is read on the device too (spans mode), or
// band j of row r (bands mode).  Every thread of a team owns a contiguous chunk of the window: of whole 16-byte quads with
// VEC (the row is read as float4 from the quad that holds a to the one that holds b, bins outside [a, b] are masked), of
// bins without.
//   Pass 1: per thread the float64 sums of p, p*(k-a), p*(k-a)^2, the valid count and the peak (largest xc, lowest bin); the
//           team's inclusive scan of the chunk sums gives every thread the float64 sum in front of its chunk (the carry) and
//           the total; the other values are reduced.
//   Pass 2: the window is read again (from L2).  Every thread finds the first and last valid bin at or above the x-dB
//           threshold in its chunk.  For the occupied bandwidth a thread counts the bins whose inclusive sum stays at or below
//           tail (obw_lo = a + that count) and the bins whose suffix sum power - exclusive sum exceeds tail (obw_hi = a +
//           that count - 1); carry and chunk sum decide that for a whole chunk at once, and only a thread whose chunk holds a
//           crossing evaluates 10^x again and walks its chunk.
// Lane 0 of the team writes the record with plain stores.  No atomics of any kind.
#pragma once
#include <hip/hip_runtime.h>

namespace ksa {
namespace measure {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int WAVE_MAX_BINS = 256;
constexpr int FLAG_MEASURED = 1, FLAG_CLIPPED = 2, FLAG_INVALID = 4;

struct Result {                     // kme_result
  long long row;
  int bin_lo, bin_hi, nvalid, flags;
  double power, m1, m2;
  int peak_bin;
  float peak_db;
  int obw_lo, obw_hi, xdb_lo, xdb_hi;
  float power_db;
  int reserved;
};
static_assert(sizeof(Result) == 80, "result record");

struct Args {
  const float* rows;
  long long row_stride;             // floats
  long long nrows, row_base;
  const unsigned char* spans;       // spans mode: the list; null in bands mode
  long long span_stride;            // bytes
  const long long* total;           // the list's count, device memory
  long long span_capacity, first;
  const int* bands;                 // bands mode: [nb][2]
  int nb;
  long long first_slot;
  Result* results;                  // [capacity]
  int capacity, nbins, margin;
  float beta, xdb;
};

struct Task {
  const float* row;
  long long id, slot;
  int a, b, flags;
};

// tasks of the launch: decided on the device in spans mode
__device__ __forceinline__ long long task_count(const Args& A) {
  if (!A.spans) return A.nrows * A.nb;
  long long lim = *A.total;
  lim = lim < A.span_capacity ? lim : A.span_capacity;
  lim = lim < (long long)A.capacity ? lim : (long long)A.capacity;
  return lim - A.first;             // <= 0: nothing to do
}

// task t of the launch; false when it is not to be measured by this form (every thread of a team decides alike)
template <bool WG>
__device__ __forceinline__ bool fetch(const Args& A, long long t, Task& k) {
  int lo, hi;
  long long r;
  k.flags = FLAG_MEASURED;
  if (A.spans) {
    k.slot = A.first + t;
    const unsigned char* rec = A.spans + k.slot * A.span_stride;
    k.id = *reinterpret_cast<const long long*>(rec);
    lo = reinterpret_cast<const int*>(rec)[2];
    hi = reinterpret_cast<const int*>(rec)[3];
    if (k.id < A.row_base || k.id - A.row_base >= A.nrows) return false;
    if (lo < 0 || hi >= A.nbins || lo > hi) return false;
    r = k.id - A.row_base;
    k.a = max(lo - A.margin, 0);
    k.b = min(hi + A.margin, A.nbins - 1);
    if (k.a != lo - A.margin || k.b != hi + A.margin) k.flags |= FLAG_CLIPPED;
  } else {
    r = t / A.nb;
    const int j = (int)(t - r * A.nb);
    k.slot = A.first_slot + t;
    k.id = A.row_base + r;
    k.a = A.bands[2 * j];
    k.b = A.bands[2 * j + 1];
  }
  if ((k.b - k.a + 1 > WAVE_MAX_BINS) != WG) return false;
  k.row = A.rows + r * A.row_stride;
  return true;
}

__device__ __forceinline__ bool valid_db(float x) { return !(x != x) && x != -INFINITY; }
__device__ __forceinline__ float clamp_db(float x) { return fminf(fmaxf(x, -500.0f), 500.0f); }
__device__ __forceinline__ double power_of(float xc) { return exp10((double)xc / 10.0); }

// fn(k, x) for the bins of units [us, ue) that lie in [a, b], in ascending order; a unit is a quad with VEC, a bin without
template <bool VEC, class F>
__device__ __forceinline__ void walk(const float* row, int us, int ue, int a, int b, F fn) {
  for (int u = us; u < ue; ++u) {
    if constexpr (VEC) {
      const float4 v = *reinterpret_cast<const float4*>(row + 4 * (long long)u);
      const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = 4 * u + j;
        if (k >= a && k <= b) fn(k, x[j]);
      }
    } else {
      fn(u, row[u]);
    }
  }
}

// is (x1, k1) a better peak than (x0, k0): the larger xc, the lower bin among equals
__device__ __forceinline__ bool better(float x1, int k1, float x0, int k0) { return x1 > x0 || (x1 == x0 && k1 < k0); }

template <bool WG, bool VEC>
__global__ __launch_bounds__(THREADS) void measure_kernel(const Args A) {
  // the workgroup form's meeting place: one entry per wave (the wave form declares nothing)
  __shared__ double sh_sum[WG ? WAVES : 1], sh_m1[WG ? WAVES : 1], sh_m2[WG ? WAVES : 1];
  __shared__ float sh_px[WG ? WAVES : 1];
  __shared__ int sh_pk[WG ? WAVES : 1], sh_nv[WG ? WAVES : 1];
  __shared__ int sh_lo[WG ? WAVES : 1], sh_hi[WG ? WAVES : 1], sh_x0[WG ? WAVES : 1], sh_x1[WG ? WAVES : 1];
  constexpr int E = VEC ? 4 : 1;
  constexpr int T = WG ? THREADS : 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tix = WG ? tid : lane;
  const long long ntasks = task_count(A);
  const long long t0 = WG ? (long long)blockIdx.x : (long long)blockIdx.x * WAVES + wave;
  const long long step = WG ? (long long)gridDim.x : (long long)gridDim.x * WAVES;

  for (long long t = t0; t < ntasks; t += step) {              // the trip count and every branch on `task` are team-uniform
    Task task;
    if (!fetch<WG>(A, t, task)) continue;
    const int a = task.a, b = task.b;
    const float* row = task.row;
    const int u0 = a / E, u1 = b / E;
    const int per = (u1 - u0 + 1 + T - 1) / T;                 // units per thread
    const int us = min(u0 + tix * per, u1 + 1), ue = min(us + per, u1 + 1);
    const int mine = max(min(ue * E - 1, b) - max(us * E, a) + 1, 0);      // bins of the window in this thread's chunk

    // pass 1
    double s = 0.0, m1 = 0.0, m2 = 0.0;
    int nv = 0, pk = 0x7FFFFFFF;
    float px = -INFINITY;
    walk<VEC>(row, us, ue, a, b, [&](int k, float x) {
      if (!valid_db(x)) return;
      const float xc = clamp_db(x);
      const double p = power_of(xc), d = (double)(k - a);
      s += p;
      m1 += p * d;
      m2 += p * d * d;
      ++nv;
      if (xc > px) {                                           // ascending k: the first of equals stays
        px = xc;
        pk = k;
      }
    });
    double inc = s;                                            // inclusive scan of the chunk sums over the wave
    for (int d = 1; d < 64; d <<= 1) {
      const double o = __shfl_up(inc, d);
      if (lane >= d) inc += o;
    }
    double carry = __shfl_up(inc, 1);
    if (lane == 0) carry = 0.0;
    double power = __shfl(inc, 63);
    for (int m = 32; m; m >>= 1) {
      m1 += __shfl_xor(m1, m);
      m2 += __shfl_xor(m2, m);
      nv += __shfl_xor(nv, m);
      const float ox = __shfl_xor(px, m);
      const int ok = __shfl_xor(pk, m);
      if (better(ox, ok, px, pk)) {
        px = ox;
        pk = ok;
      }
    }
    if constexpr (WG) {
      if (lane == 0) {
        sh_sum[wave] = power;
        sh_m1[wave] = m1;
        sh_m2[wave] = m2;
        sh_nv[wave] = nv;
        sh_px[wave] = px;
        sh_pk[wave] = pk;
      }
      __syncthreads();
      double before = 0.0;
      power = m1 = m2 = 0.0;
      nv = 0;
      px = -INFINITY;
      pk = 0x7FFFFFFF;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) {
        if (w == wave) before = power;                         // the sum of the waves in front of this one
        power += sh_sum[w];
        m1 += sh_m1[w];
        m2 += sh_m2[w];
        nv += sh_nv[w];
        if (better(sh_px[w], sh_pk[w], px, pk)) {
          px = sh_px[w];
          pk = sh_pk[w];
        }
      }
      carry += before;
    }

    // pass 2
    int cnt_lo = 0, cnt_hi = 0, x0 = 0x7FFFFFFF, x1 = -1;
    if (nv > 0) {
      const double tail = (1.0 - (double)A.beta) / 2.0 * power;
      const float thr = px - A.xdb;
      const double after = carry + s;
      // a chunk that lies wholly on one side of a crossing is counted as a whole; -1: walk it
      int whole_lo = after <= tail ? mine : carry > tail ? 0 : -1;
      int whole_hi = power - after > tail ? mine : !(power - carry > tail) ? 0 : -1;
      const bool sums = mine > 0 && (whole_lo < 0 || whole_hi < 0);
      double run = carry;
      walk<VEC>(row, us, ue, a, b, [&](int k, float x) {
        const bool ok = valid_db(x);
        const float xc = clamp_db(x);
        if (ok && xc >= thr) {
          x0 = min(x0, k);
          x1 = max(x1, k);
        }
        if (sums) {
          if (power - run > tail) ++cnt_hi;                    // the suffix sum from k on
          if (ok) run += power_of(xc);
          if (run <= tail) ++cnt_lo;                           // the sum up to and including k
        }
      });
      if (whole_lo >= 0) cnt_lo = whole_lo;
      if (whole_hi >= 0) cnt_hi = whole_hi;
    }
    for (int m = 32; m; m >>= 1) {
      cnt_lo += __shfl_xor(cnt_lo, m);
      cnt_hi += __shfl_xor(cnt_hi, m);
      x0 = min(x0, __shfl_xor(x0, m));
      x1 = max(x1, __shfl_xor(x1, m));
    }
    if constexpr (WG) {
      if (lane == 0) {
        sh_lo[wave] = cnt_lo;
        sh_hi[wave] = cnt_hi;
        sh_x0[wave] = x0;
        sh_x1[wave] = x1;
      }
      __syncthreads();
      cnt_lo = cnt_hi = 0;
      x0 = 0x7FFFFFFF;
      x1 = -1;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) {
        cnt_lo += sh_lo[w];
        cnt_hi += sh_hi[w];
        x0 = min(x0, sh_x0[w]);
        x1 = max(x1, sh_x1[w]);
      }
    }

    if (tix == 0) {
      Result r;
      r.row = task.id;
      r.bin_lo = a;
      r.bin_hi = b;
      r.nvalid = nv;
      r.flags = task.flags | (nv < b - a + 1 ? FLAG_INVALID : 0);
      r.power = power;
      r.m1 = m1;
      r.m2 = m2;
      r.peak_bin = nv > 0 ? pk : -1;
      r.peak_db = nv > 0 ? row[pk] : __int_as_float(0x7FC00000);
      r.obw_lo = nv > 0 ? a + cnt_lo : -1;
      r.obw_hi = nv > 0 ? a + cnt_hi - 1 : -1;
      r.xdb_lo = nv > 0 ? x0 : -1;
      r.xdb_hi = nv > 0 ? x1 : -1;
      r.power_db = nv > 0 ? (float)(10.0 * log10(power)) : -INFINITY;
      r.reserved = 0;
      A.results[task.slot] = r;
    }
  }
}

}  // namespace measure
}  // namespace ksa
