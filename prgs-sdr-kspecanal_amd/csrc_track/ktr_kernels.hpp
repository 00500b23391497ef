// libksa_track: the kernels of include/ksa_track.h for gfx950.  A link is eight launches on one stream:
//
//   validate  one thread per span: its rule against its predecessor, bad_spans once per wave; it also leaves the span's
//             16-byte key (row, bin_lo, bin_hi), parent[i] = i and the span's own contribution in acc[i]
//   link      one thread per span: for every present row within 1 + row_gap above it, a galloping search for the row's
//             segment, another for the first candidate inside it, then a walk that unites: in LDS where both spans belong
//             to the workgroup's 256, in memory otherwise
//   flatten   parent[i] = the root of i (in a launch of its own: nothing unites while it runs)
//   reduce    every span that is not its own root adds itself to acc[root] with integer atomics
//   mark      roots are judged (component / track) and counted per workgroup
//   scan      one workgroup: the exclusive sum of those counts, and both totals
//   compact   the rank of every track, its record when rank < capacity, labels of the roots
//   labels    labels of everyone else, from their roots
//
// parent[] is a union-find forest in which a root only ever gets pointed at a SMALLER index, by compare-and-swap.  So parents
// only decrease, every find and every retry terminates, and the root a component ends with is its lowest index whatever the
// interleaving.  Inside the link launch parent[] is touched through relaxed agent-scope atomics alone: the eight XCDs share no
// L2, a value read there may be stale, and a stale parent is still an ancestor.  No thread waits for another's progress.
//
// The lists are sorted by (row, bin_lo) and the spans of a row are disjoint, so bin_hi ascends inside a row as well: both
// searches of the link kernel are searches for the first index at which a monotone predicate turns true, done by galloping
// from where the last one ended (the next row's segment is usually a few spans away).  That is why no table of row starts is
// kept: the list itself is the index.
//
// Every kernel reads n and bad_spans from device memory (counters[3], counters[2]) and has nothing to do beyond n, or at all
// once bad_spans is non-zero; grids are sized by n_max.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ksa {
namespace track {

constexpr int THREADS = 256;
constexpr int WAVE = 64;
constexpr int WAVES = THREADS / WAVE;
constexpr int SCAN_THREADS = 1024;
constexpr int LAUNCHES = 8;
constexpr int FLAG_OPEN_END = 1;
enum { C_TRACKS = 0, C_COMPONENTS = 1, C_BAD = 2, C_N = 3 };        // the four int64 counters
enum { KIND_MEMBER = 0, KIND_FILTERED = 1, KIND_TRACK = 2 };        // what mark leaves in labels[] for compact

struct Span {
  long long row;
  int bin_lo, bin_hi, peak_bin, ndet;
  float peak_db, floor_db;
};
static_assert(sizeof(Span) == 32, "ktr_span is 32 bytes");

struct Track {
  long long row_first, row_last, peak_row, cells, sum_mid2;
  int bin_lo, bin_hi, nspans, peak_bin, mid2_first, mid2_last, first_span, flags;
  float peak_db, floor_db;
};
static_assert(sizeof(Track) == 80, "ktr_track is 80 bytes");

struct alignas(16) Key {
  long long row;
  int lo, hi;
};

// what a root gathers; acc[i] starts as span i alone
struct alignas(16) Acc {
  unsigned long long peak;      // key(peak_db) << 32 | 0xFFFFFFFF - index: the maximum is the peak span, the lowest index of equals
  unsigned long long last;      // index << 32 | bin_lo + bin_hi: the maximum is the member with the highest index
  long long cells, mid2;
  int lo, hi, nspans, pad;
};
static_assert(sizeof(Acc) == 48, "three 16-byte stores");

struct Args {
  const Span* spans;
  const long long* n_dev;       // may be null: n = n_max
  long long n_max, row_end;
  int nbins, row_gap, bin_slop, min_rows, min_spans, capacity;
  Key* keys;                    // [max_spans]
  int* parent;                  // [max_spans]
  Acc* acc;                     // [max_spans]
  int* labels;                  // [max_spans], the object's own
  int* labels_out;              // the caller's [n_max], or null
  int* block_cnt;               // [2 * blocks]: tracks, components of every workgroup of mark
  int* block_off;               // [blocks]: tracks in front of the workgroup
  long long* counters;          // [4]
  Track* tracks;                // [capacity]
};

constexpr int AGENT = __HIP_MEMORY_SCOPE_AGENT, TILE = __HIP_MEMORY_SCOPE_WORKGROUP;     // parent[] in memory, a tile's in LDS

template <int SCOPE = AGENT> __device__ __forceinline__ int load_parent(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE);
}

// the order of float32 bit patterns: -inf < ... < -0 < +0 < ... < +inf < positive NaNs
__device__ __forceinline__ unsigned peak_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The root of x, halving the path on the way.  The halving is a fetch_min, never a store: a store could raise a parent that a
// compare-and-swap has lowered meanwhile.
template <int SCOPE = AGENT> __device__ __forceinline__ int find_root(int* parent, int x) {
  int p = load_parent<SCOPE>(parent + x);
  while (p != x) {
    const int g = load_parent<SCOPE>(parent + p);
    if (g != p) __hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, SCOPE);
    x = p;
    p = g;
  }
  return x;
}

// Point the larger root at the smaller.  A failed compare-and-swap means somebody else lowered that parent: find again.
template <int SCOPE = AGENT> __device__ __forceinline__ void unite(int* parent, int a, int b) {
  for (;;) {
    a = find_root<SCOPE>(parent, a);
    b = find_root<SCOPE>(parent, b);
    if (a == b) return;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    int expected = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE))
      return;
    a = lo;
    b = hi;
  }
}

// the first index in [from, n) at which pred turns true (it stays true from there on), n when there is none
template <class Pred> __device__ __forceinline__ int first_true(int from, int n, Pred pred) {
  if (from >= n) return n;
  if (pred(from)) return from;
  int below = from, step = 1, probe = from + 1;         // pred(below) is false
  while (probe < n && !pred(probe)) {
    below = probe;
    step <<= 1;
    probe = n - below > step ? below + step : n;
  }
  int above = probe;                                    // pred(above) is true, or above == n
  while (above - below > 1) {
    const int mid = below + ((above - below) >> 1);
    if (pred(mid)) above = mid;
    else below = mid;
  }
  return above;
}

__global__ __launch_bounds__(THREADS) void validate_kernel(Args a) {
  long long n = a.n_max;
  if (a.n_dev) {
    const long long v = *a.n_dev;
    n = v < 0 ? 0 : v < a.n_max ? v : a.n_max;
  }
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (i == 0) a.counters[C_N] = n;
  bool bad = false;
  if (i < n) {
    const Span s = a.spans[i];
    bad = s.bin_lo < 0 || s.bin_lo > s.bin_hi || s.bin_hi >= a.nbins || s.row < 0 || s.row >= a.row_end;
    if (i > 0) {
      const Span p = a.spans[i - 1];
      bad = bad || !(s.row > p.row || (s.row == p.row && s.bin_lo > p.bin_lo && s.bin_lo > p.bin_hi));
    }
    Key k;
    k.row = s.row; k.lo = s.bin_lo; k.hi = s.bin_hi;
    a.keys[i] = k;
    a.parent[i] = (int)i;
    Acc c;
    const unsigned mid2 = (unsigned)s.bin_lo + (unsigned)s.bin_hi;
    c.peak = ((unsigned long long)peak_key(s.peak_db) << 32) | (0xFFFFFFFFu - (unsigned)i);
    c.last = ((unsigned long long)(unsigned)i << 32) | mid2;
    c.cells = (long long)s.bin_hi - s.bin_lo + 1;
    c.mid2 = (long long)s.bin_lo + s.bin_hi;
    c.lo = s.bin_lo; c.hi = s.bin_hi; c.nspans = 1; c.pad = 0;
    a.acc[i] = c;
  }
  const unsigned long long wave_bad = __ballot(bad);
  if (wave_bad && (threadIdx.x & (WAVE - 1)) == 0)
    atomicAdd(reinterpret_cast<unsigned long long*>(a.counters + C_BAD), (unsigned long long)__popcll(wave_bad));
}

// every later span adjacent to span i, in ascending order
template <class Edge> __device__ __forceinline__ void for_each_neighbour(const Args& a, int i, int n, Edge edge) {
  const Key* keys = a.keys;
  const Key k = keys[i];
  const long long row_max = k.row + 1 + a.row_gap;
  const long long need_hi = (long long)k.lo - a.bin_slop;       // a candidate has bin_hi >= this
  const long long limit_lo = (long long)k.hi + a.bin_slop;      // and bin_lo <= this
  long long row = k.row;
  int pos = i + 1;
  while (pos < n) {
    const int seg = first_true(pos, n, [&](int j) { return keys[j].row > row; });
    if (seg >= n) break;
    row = keys[seg].row;
    if (row > row_max) break;
    int c = first_true(seg, n, [&](int j) { const Key q = keys[j]; return q.row > row || q.hi >= need_hi; });
    for (; c < n; ++c) {
      const Key q = keys[c];
      if (q.row != row || q.lo > limit_lo) break;
      edge(c);
    }
    pos = c;
  }
}

#ifdef KTR_LINK_GLOBAL_ONLY
// The link kernel without the tile: every edge is united in memory.  Kept for the A/B of tools/track_sweep.py alone.
__global__ __launch_bounds__(THREADS) void link_kernel(Args a) {
  if (a.counters[C_BAD] != 0) return;
  const int n = (int)a.counters[C_N];
  const long long at = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (at >= n) return;
  const int i = (int)at;
  for_each_neighbour(a, i, n, [&](int c) { unite(a.parent, i, c); });
}
#else
// A workgroup's THREADS consecutive spans are a tile.  Edges inside the tile are united in a forest in LDS, edges that leave it
// in memory at once (the order of unions is free).  Then every span of the tile is united in memory with its root in the tile:
// what memory sees of a track that runs through the list is one short hop per span and a chain of tile roots, not a chain of
// spans, and most compare-and-swaps never leave the CU.
__global__ __launch_bounds__(THREADS) void link_kernel(Args a) {
  if (a.counters[C_BAD] != 0) return;
  __shared__ int tile[THREADS];
  const int n = (int)a.counters[C_N];
  const long long base = (long long)blockIdx.x * THREADS;
  if (base >= n) return;                                        // the whole workgroup
  const int t = threadIdx.x, i = (int)base + t;
  const int tile_end = (int)base + THREADS;
  tile[t] = t;
  __syncthreads();
  if (i < n)
    for_each_neighbour(a, i, n, [&](int c) {
      if (c < tile_end) unite<TILE>(tile, t, c - (int)base);
      else unite(a.parent, i, c);
    });
  __syncthreads();
  const int root = find_root<TILE>(tile, t);
  if (root != t) unite(a.parent, i, (int)base + root);
}
#endif

__global__ __launch_bounds__(THREADS) void flatten_kernel(Args a) {
  if (a.counters[C_BAD] != 0) return;
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (i >= a.counters[C_N]) return;
  const int root = find_root(a.parent, (int)i);
  __hip_atomic_store(a.parent + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the lowest index: nothing lowers it further
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m) {
  const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, m), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), m);
  return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ void add_to_root(Acc* r, const Acc& c) {
  atomicMax(&r->peak, c.peak);
  atomicMax(&r->last, c.last);
  atomicAdd(reinterpret_cast<unsigned long long*>(&r->cells), (unsigned long long)c.cells);
  atomicAdd(reinterpret_cast<unsigned long long*>(&r->mid2), (unsigned long long)c.mid2);
  atomicMin(&r->lo, c.lo);
  atomicMax(&r->hi, c.hi);
  atomicAdd(&r->nspans, c.nspans);
}

// Members add themselves to their root.  A wave whose members all have ONE root (a long track's spans are neighbours in the
// list) folds them in registers first and sends one set of atomics instead of 64.
__global__ __launch_bounds__(THREADS) void reduce_kernel(Args a) {
  if (a.counters[C_BAD] != 0) return;
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  const long long n = a.counters[C_N];
  int root = -1;
  bool member = false;
  if (i < n) {
    root = load_parent(a.parent + i);
    member = root != (int)i;
  }
  const unsigned long long members = __ballot(member);
  if (!members) return;
  const int first = __ffsll((long long)members) - 1;
  const int root0 = __shfl(root, first);
  const bool one_root = __ballot(member && root != root0) == 0;
  Acc c;
  c.peak = 0; c.last = 0; c.cells = 0; c.mid2 = 0; c.lo = 0x7FFFFFFF; c.hi = -0x7FFFFFFF - 1; c.nspans = 0; c.pad = 0;
  if (member) c = a.acc[i];
  if (!one_root) {
    if (member) add_to_root(a.acc + root, c);
    return;
  }
  for (int m = WAVE / 2; m >= 1; m >>= 1) {
    const unsigned long long peak = shfl_xor_u64(c.peak, m), last = shfl_xor_u64(c.last, m);
    c.peak = peak > c.peak ? peak : c.peak;
    c.last = last > c.last ? last : c.last;
    c.cells += (long long)shfl_xor_u64((unsigned long long)c.cells, m);
    c.mid2 += (long long)shfl_xor_u64((unsigned long long)c.mid2, m);
    const int lo = __shfl_xor(c.lo, m), hi = __shfl_xor(c.hi, m);
    c.lo = lo < c.lo ? lo : c.lo;
    c.hi = hi > c.hi ? hi : c.hi;
    c.nspans += __shfl_xor(c.nspans, m);
  }
  if ((int)(threadIdx.x & (WAVE - 1)) == first) add_to_root(a.acc + root0, c);
}

__device__ __forceinline__ long long last_row_of(const Args& a, const Acc& c) { return a.keys[(unsigned)(c.last >> 32)].row; }

__global__ __launch_bounds__(THREADS) void mark_kernel(Args a) {
  if (a.counters[C_BAD] != 0) return;
  __shared__ int wave_cnt[2 * WAVES];
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  const long long n = a.counters[C_N];
  int kind = KIND_MEMBER;
  if (i < n && load_parent(a.parent + i) == (int)i) {
    const Acc c = a.acc[i];
    const long long rows = last_row_of(a, c) - a.keys[i].row + 1;
    kind = rows >= a.min_rows && c.nspans >= a.min_spans ? KIND_TRACK : KIND_FILTERED;
  }
  if (i < n) a.labels[i] = kind;
  const unsigned long long tracks = __ballot(kind == KIND_TRACK), comps = __ballot(kind != KIND_MEMBER);
  const int wave = threadIdx.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    wave_cnt[2 * wave] = __popcll(tracks);
    wave_cnt[2 * wave + 1] = __popcll(comps);
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    int sum = 0;
    for (int w = 0; w < WAVES; ++w) sum += wave_cnt[2 * w + threadIdx.x];
    a.block_cnt[2 * blockIdx.x + threadIdx.x] = sum;
  }
}

// one workgroup: block_off[b] = the tracks of the workgroups in front of b, and both totals
__global__ __launch_bounds__(SCAN_THREADS) void scan_kernel(Args a) {
  if (a.counters[C_BAD] != 0) return;
  __shared__ long long part[SCAN_THREADS];
  __shared__ long long comp_part[SCAN_THREADS];
  const long long n = a.counters[C_N];
  const int blocks = (int)((n + THREADS - 1) / THREADS);
  const int per = (blocks + SCAN_THREADS - 1) / SCAN_THREADS;
  const int t = threadIdx.x;
  const int from = t * per < blocks ? t * per : blocks, to = from + per < blocks ? from + per : blocks;
  long long tracks = 0, comps = 0;
  for (int b = from; b < to; ++b) {
    tracks += a.block_cnt[2 * b];
    comps += a.block_cnt[2 * b + 1];
  }
  part[t] = tracks;
  comp_part[t] = comps;
  __syncthreads();
  for (int d = 1; d < SCAN_THREADS; d <<= 1) {          // inclusive scan of the per-thread sums
    const long long add = t >= d ? part[t - d] : 0, add_comp = t >= d ? comp_part[t - d] : 0;
    __syncthreads();
    part[t] += add;
    comp_part[t] += add_comp;
    __syncthreads();
  }
  long long run = part[t] - tracks;
  for (int b = from; b < to; ++b) {
    a.block_off[b] = (int)run;
    run += a.block_cnt[2 * b];
  }
  if (t == SCAN_THREADS - 1) {
    a.counters[C_TRACKS] = part[t];
    a.counters[C_COMPONENTS] = comp_part[t];
  }
}

__global__ __launch_bounds__(THREADS) void compact_kernel(Args a) {
  if (a.counters[C_BAD] != 0) return;
  __shared__ int wave_cnt[WAVES];
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  const long long n = a.counters[C_N];
  if ((long long)blockIdx.x * THREADS >= n) return;     // the whole workgroup: block_off has no entry for it
  const int kind = i < n ? a.labels[i] : KIND_MEMBER;
  const bool track = kind == KIND_TRACK;
  const unsigned long long mask = __ballot(track);
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  if (lane == 0) wave_cnt[wave] = __popcll(mask);
  __syncthreads();
  int rank = a.block_off[blockIdx.x] + __popcll(mask & ((1ull << lane) - 1));
  for (int w = 0; w < wave; ++w) rank += wave_cnt[w];
  if (kind == KIND_FILTERED) a.labels[i] = -1;
  if (!track) return;
  a.labels[i] = rank;
  if (rank >= a.capacity) return;
  const Acc c = a.acc[i];
  const unsigned peak_at = 0xFFFFFFFFu - (unsigned)c.peak;
  const Span p = a.spans[peak_at];
  const Key k = a.keys[i];
  Track r;
  r.row_first = k.row;
  r.row_last = last_row_of(a, c);
  r.peak_row = p.row;
  r.cells = c.cells;
  r.sum_mid2 = c.mid2;
  r.bin_lo = c.lo;
  r.bin_hi = c.hi;
  r.nspans = c.nspans;
  r.peak_bin = p.peak_bin;
  r.mid2_first = k.lo + k.hi;
  r.mid2_last = (int)(unsigned)c.last;
  r.first_span = (int)i;
  r.flags = r.row_last + a.row_gap + 1 >= a.row_end ? FLAG_OPEN_END : 0;
  r.peak_db = p.peak_db;
  r.floor_db = p.floor_db;
  a.tracks[rank] = r;
}

// labels of the members from their roots; -1 everywhere when nothing was linked, and from n on
__global__ __launch_bounds__(THREADS) void labels_kernel(Args a) {
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (i >= a.n_max) return;
  int v = -1;
  if (a.counters[C_BAD] == 0 && i < a.counters[C_N]) {
    const int root = load_parent(a.parent + i);
    v = a.labels[root];                                 // a root's own entry is final since compact; only members are written here
    if (root != (int)i) a.labels[i] = v;
  } else {
    a.labels[i] = -1;
  }
  if (a.labels_out) a.labels_out[i] = v;
}

}  // namespace track
}  // namespace ksa
