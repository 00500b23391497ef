// libksa_pulse: the time-domain pulse detector and pulse list of include/ksa_pulse.h for gfx950.
//
// Both forms of the header run the same kernels on a flat list of tiles: a tile is TILE = 2048 consecutive samples of one block
// (the stream form is one block whose past comes from the object's carried state), 256 threads, eight samples per thread.
// Every quantity that crosses a thread, a tile or a call is an integer or a pick among integers, and every merge below is
// associative, so neither the tile nor the grid nor the cut of a stream can enter a result.
//
//  1. env_kernel: one workgroup per tile.  It brings q of the tile and of the W-1 samples before it into LDS (16-byte loads
//     where a vector lies wholly inside the span, single samples at its ends, the carried q history or zeros before the block),
//     turns it into an inclusive prefix sum in place (a serial sum per thread over a contiguous stretch, a workgroup scan of
//     the 256 sums, a second serial pass), and reads S[n] = P[n] - P[n-W] off it.  S goes to the object's work buffer and,
//     where asked, to the caller's.  The tile's summary is its last op that is not HOLD.
//  2. state_kernel: one workgroup per block scans the summaries ("the later op that is not HOLD wins", as a maximum over
//     (index, op) keys) from the carried state to the hysteresis state at every tile's start.
//  3. runs_kernel<false>: one workgroup per tile.  The same scan over the ops of the samples gives active[n]; a segmented scan
//     of per-sample records (an inactive sample resets, an active one merges) gives at every sample the record of its run from
//     the run's start or the tile's.  The thread that holds a run's first inactive sample owns the run: it is the tile's head
//     (it entered from the left), or an interior run, counted when it has min_len samples.  The run active at the tile's last
//     sample is the tile's tail, or, when it entered from the left, the mark "active throughout".
//  4. stitch_kernel: one workgroup for the launch.  A segmented scan over the tiles (a tile that is not active throughout
//     resets and contributes its tail) gives the open run at every tile's end, from the carried open run on; a tile whose
//     in-state is active and which is not active throughout completes that run with its head.  Counts per tile (the completed
//     run, the interior runs, the run a block's end closes) are scanned into slots behind the records the list already holds;
//     the stitched records are written, the totals and the carried state updated.
//  5. runs_kernel<true> repeats the tiles that have interior runs and a slot inside the buffer, and stores each record at its
//     place: whatever order the workgroups run in, the list is in ascending (block, start) order, and no atomic is involved.
//  6. hist_kernel (stream form): the last W-1 values of q and the last unpacked sample for the next call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../csrc_shared/ksa_iq.hpp"

namespace ksa {
namespace pulse {

constexpr int THREADS = 256;
constexpr int PER = 8;                              // samples per thread of the run stage
constexpr int TILE = THREADS * PER;                 // samples per workgroup
constexpr int REC_WORDS = 8;                        // kpl_pulse: 64 bytes as int64 words
constexpr int OP_HOLD = 0, OP_SET = 1, OP_CLEAR = 2;
constexpr int FLAG_OPEN_END = 1;
// the object's device words: both totals and what a stream carries from call to call
constexpr int ST_TOTAL = 0, ST_ACTIVE = 1, ST_STATE = 2, ST_OPEN = 3, ST_LAST = 9, ST_WORDS = 10;
constexpr float UNIT = 1073741824.0f;               // 2^30

// the partial record of a run; start follows from where the run ends
struct Rec {
  long long len, energy, peak, peak_pos, dre, dim;
};
__host__ __device__ __forceinline__ Rec rec_none() { return Rec{0, 0, -1, 0x7fffffffffffffffll, 0, 0}; }
// a lies before b: sums add, the larger peak wins, the earlier position among equals
__device__ __forceinline__ Rec merge(const Rec& a, const Rec& b) {
  const bool tb = b.peak > a.peak || (b.peak == a.peak && b.peak_pos < a.peak_pos);
  return Rec{a.len + b.len, a.energy + b.energy, tb ? b.peak : a.peak, tb ? b.peak_pos : a.peak_pos, a.dre + b.dre, a.dim + b.dim};
}
// an element of the segmented scan: f = a reset lies inside, v = the record since the last reset
struct Seg {
  int f;
  Rec v;
};
__device__ __forceinline__ Seg seg_none() { return Seg{0, rec_none()}; }
__device__ __forceinline__ Seg seg_combine(const Seg& a, const Seg& b) { return Seg{a.f | b.f, b.f ? b.v : merge(a.v, b.v)}; }

struct Args {
  const void* in;                   // the call's raw samples (block 0)
  const long long* qhist;           // stream form: q of the W-1 samples before the call; null in the block form
  long long* state;                 // [ST_WORDS]
  long long* S;                     // work: block b, sample i at [b len + i]
  long long* env;                   // dense S or null: [b out_stride + i]
  long long* events;                // [capacity][REC_WORDS]
  int* summary;                     // per tile: its last op that is not HOLD
  int* state_in;                    // per tile: active at the tile's start
  int* info;                        // per tile: 1 = entered active and active throughout
  int* cnt;                         // per tile: interior runs of min_len samples or more
  long long* act;                   // per tile: their samples
  long long* off;                   // per tile: the slot of its first interior run
  Rec* head;                        // per tile: the run that entered from the left, up to its end or the tile's
  Rec* tail;                        // per tile: the run that began inside and is active at the tile's last sample
  long long block_stride;           // samples
  long long out_stride;             // samples
  long long ntiles;                 // tiles of the launch
  long long pos_base;               // position of sample 0: samples_in of the stream, 0 in the block form
  long long thr_on, thr_off;
  int fmt;
  float u8_offset, u8_inv_scale;
  int len;                          // samples per block
  int tiles;                        // tiles per block
  int W, min_len, capacity;
  int stream;                       // 1: the stream form (block is -1, the carried state is read and written)
  int final;                        // 1: the end of a block closes the open run
};

// One rounding per operation: a product formed here carries no licence to be contracted into a fused multiply-add with the
// sum it feeds (the plain __fmul_rn is an ordinary product to the compiler, and the default contraction would fuse it).
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
__device__ __forceinline__ long long q_of(const float2 x) {
  const float p = add_rn(mul_rn(x.x, x.x), mul_rn(x.y, x.y));
  return (long long)rintf(mul_rn(fminf(p, 4.0f), UNIT));
}
__device__ __forceinline__ long long d_of(const float v) { return (long long)rintf(mul_rn(fminf(fmaxf(v, -4.0f), 4.0f), UNIT)); }
__device__ __forceinline__ int op_of(const Args& a, long long s) { return s >= a.thr_on ? OP_SET : s < a.thr_off ? OP_CLEAR : OP_HOLD; }

__device__ __forceinline__ int shfl_up_t(int v, int d) { return __shfl_up(v, d); }
__device__ __forceinline__ long long shfl_up_t(long long v, int d) { return __shfl_up(v, d); }
__device__ __forceinline__ Seg shfl_up_t(const Seg& s, int d) {
  return Seg{__shfl_up(s.f, d), Rec{__shfl_up(s.v.len, d), __shfl_up(s.v.energy, d), __shfl_up(s.v.peak, d), __shfl_up(s.v.peak_pos, d),
                                    __shfl_up(s.v.dre, d), __shfl_up(s.v.dim, d)}};
}

// exclusive scan of x over the workgroup in thread order under op (associative, none its identity); *all = the whole
template <class T, class Op> __device__ __forceinline__ T block_scan_excl(const T x, const T none, Op op, T* all = nullptr) {
  __shared__ T wave_tot[THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T inc = x;
  for (int d = 1; d < 64; d <<= 1) {
    const T o = shfl_up_t(inc, d);
    if (lane >= d) inc = op(o, inc);
  }
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  T before = none, whole = none;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) {
    if (w < wave) before = op(before, wave_tot[w]);
    whole = op(whole, wave_tot[w]);
  }
  const T prev = shfl_up_t(inc, 1);
  if (all) *all = whole;
  __syncthreads();                                              // wave_tot is free for the next scan
  return lane == 0 ? before : op(before, prev);
}
__device__ __forceinline__ int max_op(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int add_i(int a, int b) { return a + b; }
__device__ __forceinline__ long long add_ll(long long a, long long b) { return a + b; }

// raw samples [r0, r0 + n) of the block at base, all of them inside the block: f(j, sample) for j = 0 .. n-1, 16-byte loads
// where a vector lies wholly inside the range
template <int FMT, class F> __device__ __forceinline__ void for_samples(const Args& a, const char* base, int r0, int n, F f) {
  constexpr int V = iq::Fmt<FMT>::PER_VEC, BYTES = iq::Fmt<FMT>::BYTES;
  if (n <= 0) return;
  const char* p0 = base + (long long)r0 * BYTES;
  const int mis = (int)((reinterpret_cast<uintptr_t>(p0) & 15u) / BYTES);
  const char* v0 = p0 - mis * BYTES;                            // 16-byte aligned; only read where a whole vector is inside
  const int nvec = (n + mis + V - 1) / V;
  for (int g = threadIdx.x; g < nvec; g += THREADS) {
    const int j0 = V * g - mis;
    if (j0 >= 0 && j0 + V <= n) {
      const uint4 w = *reinterpret_cast<const uint4*>(v0 + (size_t)g * 16);
#pragma unroll
      for (int e = 0; e < V; ++e) f(j0 + e, iq::sample_of<FMT>(w, e, a));
    } else {
      for (int e = 0; e < V; ++e) {
        const int j = j0 + e;
        if (j >= 0 && j < n) f(j, iq::sample_at<FMT>(base, r0 + j, a));
      }
    }
  }
}

__device__ __forceinline__ const char* block_base(const Args& a, long long b, int bytes) {
  return static_cast<const char*>(a.in) + (size_t)(b * a.block_stride) * bytes;
}

template <int FMT> __global__ __launch_bounds__(THREADS) void env_kernel(const Args a) {
  extern __shared__ __attribute__((aligned(16))) long long kpl_lds[];      // [0] = 0, then the prefix over TILE + W - 1 samples
  __shared__ int best_of[THREADS / 64];
  const int tid = threadIdx.x, W = a.W;
  const long long w = blockIdx.x, b = w / a.tiles;
  const int i0 = (int)(w - b * a.tiles) * TILE;
  const int count = min(TILE, a.len - i0);
  const int L = count + W - 1, u0 = i0 - (W - 1);               // the span: samples u0 .. i0 + count - 1 of the block
  const int nh = min(L, max(0, -u0));                           // leading ones that lie before the block
  long long* P = kpl_lds + 1;
  if (tid == 0) kpl_lds[0] = 0;
  for (int s = tid; s < nh; s += THREADS) P[s] = a.qhist ? a.qhist[i0 + s] : 0;
  for_samples<FMT>(a, block_base(a, b, iq::Fmt<FMT>::BYTES), u0 + nh, L - nh, [&](int j, const float2 x) { P[nh + j] = q_of(x); });
  __syncthreads();
  const int E = (L + THREADS - 1) / THREADS, lo = min(L, tid * E), hi = min(L, lo + E);
  long long sum = 0;
  for (int s = lo; s < hi; ++s) sum += P[s];
  long long run = block_scan_excl<long long>(sum, 0ll, add_ll);
  for (int s = lo; s < hi; ++s) {
    run += P[s];
    P[s] = run;
  }
  __syncthreads();
  int best = 0;                                                 // (index + 1, op) of the tile's last op that is not HOLD
  for (int j = tid; j < count; j += THREADS) {
    const long long s = kpl_lds[W + j] - kpl_lds[j];
    a.S[b * a.len + i0 + j] = s;
    if (a.env) a.env[b * a.out_stride + i0 + j] = s;
    const int op = op_of(a, s);
    if (op) best = ((j + 1) << 2) | op;                         // j ascends
  }
  for (int m = 32; m; m >>= 1) best = max(best, __shfl_xor(best, m));
  if ((tid & 63) == 0) best_of[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
    for (int v = 1; v < THREADS / 64; ++v) best = max(best, best_of[v]);
    a.summary[w] = best & 3;
  }
}

__global__ __launch_bounds__(THREADS) void state_kernel(const Args a) {
  __shared__ int carry;
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  if (tid == 0) carry = a.stream ? (int)a.state[ST_STATE] : 0;
  __syncthreads();
  for (int first = 0; first < a.tiles; first += THREADS) {
    const int k = first + tid;
    const int sm = k < a.tiles ? a.summary[b * a.tiles + k] : 0;
    int all = 0;
    const int ex = block_scan_excl<int>(sm ? (((tid + 1) << 2) | sm) : 0, 0, max_op, &all);
    const int c = carry;
    if (k < a.tiles) a.state_in[b * a.tiles + k] = ex ? ((ex & 3) == OP_SET) : c;
    __syncthreads();
    if (tid == 0 && all) carry = (all & 3) == OP_SET;
    __syncthreads();
  }
}

__device__ __forceinline__ void write_record(const Args& a, long long slot, const Rec& r, long long end, long long block, int flags) {
  if (slot >= (long long)a.capacity) return;
  long long* e = a.events + slot * REC_WORDS;
  e[0] = end - r.len;
  e[1] = r.len;
  e[2] = r.energy;
  e[3] = r.peak;
  e[4] = r.peak_pos;
  e[5] = r.dre;
  e[6] = r.dim;
  e[7] = (long long)(((unsigned long long)(unsigned)flags << 32) | (unsigned long long)(unsigned)(int)(a.stream ? -1 : block));
}

template <int FMT, bool EMIT> __global__ __launch_bounds__(THREADS) void runs_kernel(const Args a) {
  __shared__ float2 x[TILE + 1];                                // x[j + 1] = sample i0 + j, x[0] its predecessor
  __shared__ Rec sh_head, sh_tail;
  __shared__ int sh_info;
  const int tid = threadIdx.x;
  const long long w = blockIdx.x;
  if (EMIT) {
    if (a.cnt[w] == 0 || a.off[w] >= (long long)a.capacity) return;        // workgroup-uniform
  }
  const long long b = w / a.tiles;
  const int i0 = (int)(w - b * a.tiles) * TILE;
  const int count = min(TILE, a.len - i0);
  const int lead = i0 > 0 ? 1 : 0;
  for_samples<FMT>(a, block_base(a, b, iq::Fmt<FMT>::BYTES), i0 - lead, count + lead, [&](int j, const float2 v) { x[j + 1 - lead] = v; });
  if (tid == 0) {
    if (!lead) {
      const unsigned long long bits = a.stream ? (unsigned long long)a.state[ST_LAST] : 0ull;
      x[0] = make_float2(__uint_as_float((unsigned)(bits & 0xffffffffull)), __uint_as_float((unsigned)(bits >> 32)));
    }
    sh_head = rec_none();
    sh_tail = rec_none();
    sh_info = 0;
  }
  __syncthreads();

  const int j0 = tid * PER;
  const long long pos0 = a.pos_base + i0 + j0;
  long long sv[PER];
  int last_op = 0, ops = 0;                                     // ops: two bits per sample
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    sv[e] = j0 + e < count ? a.S[b * a.len + i0 + j0 + e] : 0;
    const int op = j0 + e < count ? op_of(a, sv[e]) : OP_HOLD;
    ops |= op << (2 * e);
    if (op) last_op = op;
  }
  const int ex_op = block_scan_excl<int>(last_op ? (((tid + 1) << 2) | last_op) : 0, 0, max_op);
  const bool st_in = ex_op ? ((ex_op & 3) == OP_SET) : (a.state_in[w] != 0);
  unsigned active = 0;                                          // one bit per sample of this thread
  {
    bool st = st_in;
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const int op = (ops >> (2 * e)) & 3;
      if (op) st = op == OP_SET;
      if (st && j0 + e < count) active |= 1u << e;
    }
  }
  // the record of sample e alone; its pair with the sample before it counts when that one is active too
  auto value = [&](int e) {
    const float2 c = x[j0 + e + 1], y = x[j0 + e];
    const bool pair = e ? ((active >> (e - 1)) & 1u) : st_in;
    const float re = add_rn(mul_rn(c.x, y.x), mul_rn(c.y, y.y));
    const float im = sub_rn(mul_rn(c.y, y.x), mul_rn(c.x, y.y));
    return Rec{1, q_of(c), sv[e], pos0 + e, pair ? d_of(re) : 0, pair ? d_of(im) : 0};
  };
  Seg mine = seg_none();
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    if (j0 + e >= count) continue;
    if ((active >> e) & 1u) mine.v = merge(mine.v, value(e));
    else mine = Seg{1, rec_none()};
  }
  // a tile that starts inactive starts behind a reset: only a run that entered from the left has f = 0
  const Seg before = seg_combine(Seg{a.state_in[w] ? 0 : 1, rec_none()}, block_scan_excl<Seg>(mine, seg_none(), seg_combine));

  // walk the thread's samples from the scan's state; interior(record, index of the run's first inactive sample)
  auto walk = [&](bool keep_edges, auto interior) {
    Seg r = before;
    bool prev = st_in;
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const int j = j0 + e;
      if (j >= count) continue;
      const bool on = (active >> e) & 1u;
      if (on) {
        r.v = merge(r.v, value(e));
        if (j == count - 1 && keep_edges) {                     // the run leaves the tile
          if (r.f) sh_tail = r.v;
          else { sh_head = r.v; sh_info = 1; }
        }
      } else {
        if (prev) {
          if (r.f) interior(r.v, j);
          else if (keep_edges) sh_head = r.v;                   // entered from the left and ends here
        }
        r = Seg{1, rec_none()};
      }
      prev = on;
    }
  };
  int n_mine = 0;
  long long act_mine = 0;
  walk(!EMIT, [&](const Rec& v, int) {
    if (v.len >= a.min_len) {
      ++n_mine;
      act_mine += v.len;
    }
  });
  int n_all = 0;
  const int n_before = block_scan_excl<int>(n_mine, 0, add_i, &n_all);
  if (!EMIT) {
    long long act_all = 0;
    (void)block_scan_excl<long long>(act_mine, 0ll, add_ll, &act_all);     // its barriers also order sh_head and sh_tail
    if (tid == 0) {
      a.cnt[w] = n_all;
      a.act[w] = act_all;
      a.head[w] = sh_head;
      a.tail[w] = sh_tail;
      a.info[w] = sh_info;
    }
  } else {
    long long slot = a.off[w] + n_before;
    walk(false, [&](const Rec& v, int j) {
      if (v.len >= a.min_len) write_record(a, slot++, v, a.pos_base + i0 + j, b, 0);
    });
  }
}

__global__ __launch_bounds__(THREADS) void stitch_kernel(const Args a) {
  const int tid = threadIdx.x;
  const long long NT = a.ntiles;
  const long long total0 = a.state[ST_TOTAL];
  Rec carry = rec_none();
  if (a.stream) {
    const long long* o = a.state + ST_OPEN;
    carry = Rec{o[0], o[1], o[2], o[3], o[4], o[5]};
  }
  if (NT == 0) {                                                // kpl_flush: close the carried run
    if (tid == 0 && a.stream && a.final && a.state[ST_STATE]) {
      if (carry.len >= a.min_len) {
        write_record(a, total0, carry, a.pos_base, 0, FLAG_OPEN_END);
        a.state[ST_TOTAL] = total0 + 1;
        a.state[ST_ACTIVE] += carry.len;
      }
      const Rec none = rec_none();
      a.state[ST_STATE] = 0;
      long long* o = a.state + ST_OPEN;
      o[0] = none.len; o[1] = none.energy; o[2] = none.peak; o[3] = none.peak_pos; o[4] = none.dre; o[5] = none.dim;
    }
    return;
  }
  const long long C = (NT + THREADS - 1) / THREADS, lo = min(NT, tid * C), hi = min(NT, lo + C);
  auto elem = [&](long long k) {
    const bool through = a.info[k] & 1;
    return Seg{through ? 0 : 1, through ? a.head[k] : a.tail[k]};
  };
  Seg mine = seg_none();
  for (long long k = lo; k < hi; ++k) mine = seg_combine(mine, elem(k));
  const Seg before = seg_combine(Seg{0, carry}, block_scan_excl<Seg>(mine, seg_none(), seg_combine));

  Seg last = before;                                            // the open run at the end of this thread's tiles
  long long n = 0, n_act = 0;
  auto walk = [&](bool emit, long long slot0) {
    Seg X = before;
    n = 0;
    n_act = 0;
    for (long long k = lo; k < hi; ++k) {
      const long long b = k / a.tiles;
      const int t = (int)(k - b * a.tiles);
      const bool through = a.info[k] & 1;
      if (a.state_in[k] && !through) {                          // the run that was open ends in this tile, with the tile's head
        const Rec h = a.head[k];
        const Rec r = merge(X.v, h);
        if (r.len >= a.min_len) {
          if (emit) write_record(a, slot0 + n, r, a.pos_base + (long long)t * TILE + h.len, b, 0);
          ++n;
          n_act += r.len;
        }
      }
      if (emit) a.off[k] = slot0 + n;
      n += a.cnt[k];
      n_act += a.act[k];
      X = seg_combine(X, elem(k));
      if (a.final && t == a.tiles - 1) {                        // the block ends: close what is open
        if (through || a.tail[k].len > 0) {
          if (X.v.len >= a.min_len) {
            if (emit) write_record(a, slot0 + n, X.v, a.pos_base + a.len, b, FLAG_OPEN_END);
            ++n;
            n_act += X.v.len;
          }
        }
        X = Seg{1, rec_none()};
      }
    }
    last = X;
  };
  walk(false, 0);
  long long n_all = 0, act_all = 0;
  const long long n_before = block_scan_excl<long long>(n, 0ll, add_ll, &n_all);
  (void)block_scan_excl<long long>(n_act, 0ll, add_ll, &act_all);
  walk(true, total0 + n_before);
  if (tid == 0) {
    a.state[ST_TOTAL] = total0 + n_all;
    a.state[ST_ACTIVE] += act_all;
  }
  if (a.stream && !a.final && hi == NT && lo < hi) {            // the thread that holds the last tile carries the stream on
    const bool open = (a.info[NT - 1] & 1) || a.tail[NT - 1].len > 0;
    const Rec v = open ? last.v : rec_none();
    a.state[ST_STATE] = open ? 1 : 0;
    long long* o = a.state + ST_OPEN;
    o[0] = v.len; o[1] = v.energy; o[2] = v.peak; o[3] = v.peak_pos; o[4] = v.dre; o[5] = v.dim;
  }
}

// the stream's q history and last sample after a call of a.len samples (dst is not a.qhist)
template <int FMT> __global__ __launch_bounds__(THREADS) void hist_kernel(const Args a, long long* dst) {
  const int i = blockIdx.x * THREADS + threadIdx.x;
  const char* base = static_cast<const char*>(a.in);
  if (i < a.W - 1) {
    const int idx = a.len - (a.W - 1) + i;
    dst[i] = idx < 0 ? a.qhist[a.W - 1 + idx] : q_of(iq::sample_at<FMT>(base, idx, a));
  }
  if (i == 0) {
    const float2 v = iq::sample_at<FMT>(base, a.len - 1, a);
    a.state[ST_LAST] = (long long)(((unsigned long long)__float_as_uint(v.y) << 32) | (unsigned long long)__float_as_uint(v.x));
  }
}

}  // namespace pulse
}  // namespace ksa
