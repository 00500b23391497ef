// Kernels of libksa_mask (include/ksa_mask.h): the mask check pass, the ordered event compaction and the element-wise merge.
//
// check_kernel<VEC>: one workgroup takes a strip of THREADS * E adjacent bins (E = 4 with 16-byte loads, 1 with 4-byte loads)
// for a chunk of input rows.  A lane keeps the limit lines of its E bins and three uint32 hit counters per bin in registers
// for the whole chunk (a chunk is at most 65 536 rows, so a counter cannot wrap) and flushes the non-zero ones with 64-bit
// integer atomics at the end.  Lanes walk ADJACENT bins of a row; where the strip is narrower than the workgroup the next
// lanes take the next row (lpr lanes per row, a power of two, so a lane keeps its bins).  Per row a wave takes ONE ballot of
// "any over, under or NaN in my lanes": in the common case nothing crossed a line and the wave goes on to the next row.  Only
// a wave that saw something counts, reduces the three counts and the peak key over the lanes that share a row (xor
// butterflies inside the aligned segment of min(lpr, 64) lanes) and adds the result to the row's scratch record in global
// memory: three 32-bit integer atomicAdds and one 64-bit atomicMax, all order-free.
//
// The peak key: the excess's float bits in the high word (the excess is >= 0, so integer order is float order), and in the
// low word (0x7FFFFFFF - bin) << 1 | kind, so that among equal excesses the lowest bin wins; a bin is over or under, never
// both, so the kind bit never decides between bins.  Key 0 = no over or under bin.
//
// count_kernel / scatter_kernel: the per-row records in row order, 256 rows per workgroup.  The first decides which rows are
// events, writes row_event and the workgroup's event count, and snapshots events_total; the second places every event
// behind the snapshot + the counts of the workgroups before it + an in-workgroup scan (ballots), so the buffer is in
// ascending row order whatever order the workgroups run in, and the last workgroup advances events_total.
#pragma once
#include <hip/hip_runtime.h>

namespace ksa {
namespace mask {

constexpr int THREADS = 256;
constexpr int ROWS_UNROLL = 4;      // independent row loads in flight per lane
constexpr int SCAN_THREADS = 256;   // rows per workgroup of the compaction

struct RowRec {                     // 24 bytes per row of a launch, cleared per launch
  unsigned long long key;
  unsigned nover, nunder, nnan, pad;
};
static_assert(sizeof(RowRec) == 24, "scratch record");

struct Event {                      // ksm_event
  long long row;
  int nover, nunder, nnan, peak_bin;
  float peak_excess;
  int peak_kind;
};
static_assert(sizeof(Event) == 32, "event record");

struct CheckArgs {
  const float* rows;
  long long row_stride;             // floats
  const float* upper;
  const float* lower;
  unsigned long long* hits;         // [3][nbins]
  RowRec* rec;                      // [nrows]
  int nrows, nbins, nstrips, chunk_rows;
};

__device__ __forceinline__ unsigned long long peak_key(float excess, int bin, unsigned kind) {
  return ((unsigned long long)__float_as_uint(excess) << 32) | (unsigned long long)(((0x7FFFFFFFu - (unsigned)bin) << 1) | kind);
}

template <bool VEC>
__global__ __launch_bounds__(THREADS) void check_kernel(const CheckArgs a) {
  constexpr int E = VEC ? 4 : 1;
  constexpr int SB = THREADS * E;                       // bins of a full strip
  const int tid = threadIdx.x, lane = tid & 63;
  const int strip = blockIdx.x % a.nstrips, chunk = blockIdx.x / a.nstrips;
  const int bin0 = strip * SB;
  const int nbe = min(SB, a.nbins - bin0) / E;          // elements (floats or float4) of a row that this strip holds
  const long long row0 = (long long)chunk * a.chunk_rows;
  const int nr = (int)min((long long)a.chunk_rows, (long long)a.nrows - row0);

  int lpr = 1;                                          // lanes per row: a power of two, nbe <= lpr <= THREADS
  while (lpr < nbe) lpr <<= 1;
  const int rpp = THREADS / lpr;                        // rows per pass of the workgroup
  const int seg = min(lpr, 64);                         // lanes of a wave that share a row
  const int q = tid & (lpr - 1), rr = tid / lpr;
  const bool qok = q < nbe;
  const int b0 = bin0 + (qok ? q : 0) * E;

  float up[E], lo[E];
  unsigned cnt[3][E];
#pragma unroll
  for (int j = 0; j < E; ++j) {
    up[j] = a.upper[b0 + j];
    lo[j] = a.lower[b0 + j];
    cnt[0][j] = cnt[1][j] = cnt[2][j] = 0;
  }

  const float* p = a.rows + (row0 + rr) * a.row_stride + b0;
  const long long step = (long long)rpp * a.row_stride;
  for (int rb = 0; rb < nr; rb += rpp * ROWS_UNROLL, p += step * ROWS_UNROLL) {     // trip counts are workgroup-uniform
    float x[ROWS_UNROLL][E];
    bool ok[ROWS_UNROLL];
#pragma unroll
    for (int u = 0; u < ROWS_UNROLL; ++u) {
      ok[u] = qok && rb + rr + u * rpp < nr;
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
      bool over[E], under[E], nan[E];
      bool any = false;
#pragma unroll
      for (int j = 0; j < E; ++j) {
        over[j] = ok[u] && x[u][j] > up[j];
        under[j] = ok[u] && x[u][j] < lo[j];
        nan[j] = ok[u] && x[u][j] != x[u][j];
        any = any || over[j] || under[j] || nan[j];
      }
      if (__ballot(any) == 0ull) continue;              // wave-uniform: the quiet case streams on

      unsigned packed = 0;                              // nover | nunder << 10 | nnan << 20: at most 256 each per segment
      unsigned long long key = 0;
#pragma unroll
      for (int j = 0; j < E; ++j) {
        unsigned long long k = 0;
        if (over[j]) {
          cnt[0][j] += 1;
          packed += 1u;
          k = peak_key(__fsub_rn(x[u][j], up[j]), b0 + j, 0u);
        }
        if (under[j]) {
          cnt[1][j] += 1;
          packed += 1u << 10;
          k = peak_key(__fsub_rn(lo[j], x[u][j]), b0 + j, 1u);
        }
        if (nan[j]) {
          cnt[2][j] += 1;
          packed += 1u << 20;
        }
        key = k > key ? k : key;
      }
      for (int m = 1; m < seg; m <<= 1) {
        packed += __shfl_xor(packed, m);
        const unsigned long long other = __shfl_xor(key, m);
        key = other > key ? other : key;
      }
      if ((lane & (seg - 1)) == 0 && packed != 0) {     // packed != 0 only for a row that exists
        RowRec* r = a.rec + (row0 + rb + rr + u * rpp);
        const unsigned no = packed & 1023u, nu = (packed >> 10) & 1023u, nn = packed >> 20;
        if (no) atomicAdd(&r->nover, no);
        if (nu) atomicAdd(&r->nunder, nu);
        if (nn) atomicAdd(&r->nnan, nn);
        if (key) atomicMax(&r->key, key);
      }
    }
  }

  if (qok) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int j = 0; j < E; ++j)
        if (cnt[k][j]) atomicAdd(&a.hits[(long long)k * a.nbins + b0 + j], (unsigned long long)cnt[k][j]);
  }
}

struct ScanArgs {
  const RowRec* rec;                // [nrows]
  int nrows, min_bins, capacity;
  unsigned char* row_event;         // [nrows] or null
  int* block_counts;                // [ceil(nrows / SCAN_THREADS)]
  long long* events_total;
  long long* snapshot;              // events_total as it was before this launch
  Event* events;                    // [capacity]
  long long row_base;               // running index of row 0 of this launch
};

__device__ __forceinline__ bool is_event(const RowRec& r, int min_bins) {
  return r.nover + r.nunder >= (unsigned)min_bins || r.nnan > 0;
}

__global__ __launch_bounds__(SCAN_THREADS) void count_kernel(const ScanArgs a) {
  const int i = blockIdx.x * SCAN_THREADS + threadIdx.x;
  bool ev = false;
  if (i < a.nrows) {
    ev = is_event(a.rec[i], a.min_bins);
    if (a.row_event) a.row_event[i] = ev ? 1 : 0;
  }
  const int c = __syncthreads_count(ev);
  if (threadIdx.x == 0) {
    a.block_counts[blockIdx.x] = c;
    if (blockIdx.x == 0) *a.snapshot = *a.events_total;
  }
}

__global__ __launch_bounds__(SCAN_THREADS) void scatter_kernel(const ScanArgs a) {
  constexpr int WAVES = SCAN_THREADS / 64;
  __shared__ long long before[WAVES];
  __shared__ int wave_events[WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long part = 0;
  for (int b = tid; b < (int)blockIdx.x; b += SCAN_THREADS) part += a.block_counts[b];
  for (int m = 32; m; m >>= 1) part += __shfl_xor(part, m);
  const int i = blockIdx.x * SCAN_THREADS + tid;
  RowRec r = {0ull, 0u, 0u, 0u, 0u};
  bool ev = false;
  if (i < a.nrows) {
    r = a.rec[i];
    ev = is_event(r, a.min_bins);
  }
  const unsigned long long votes = __ballot(ev);
  if (lane == 0) {
    before[wave] = part;
    wave_events[wave] = __popcll(votes);
  }
  __syncthreads();
  long long pos = *a.snapshot;
  int mine = __popcll(votes & ((1ull << lane) - 1ull)), all = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    pos += before[w];
    if (w < wave) mine += wave_events[w];
    all += wave_events[w];
  }
  if (blockIdx.x == gridDim.x - 1 && tid == 0) *a.events_total = pos + all;
  pos += mine;
  if (ev && pos < (long long)a.capacity) {
    Event e;
    e.row = a.row_base + i;
    e.nover = (int)r.nover;
    e.nunder = (int)r.nunder;
    e.nnan = (int)r.nnan;
    if (r.key) {
      const unsigned low = (unsigned)r.key;
      e.peak_bin = (int)(0x7FFFFFFFu - (low >> 1));
      e.peak_excess = __uint_as_float((unsigned)(r.key >> 32));
      e.peak_kind = (int)(low & 1u);
    } else {
      e.peak_bin = -1;
      e.peak_excess = 0.0f;
      e.peak_kind = -1;
    }
    a.events[pos] = e;
  }
}

__global__ void merge_kernel(long long* hits, const long long* other, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    hits[i] += other[i];
}

}  // namespace mask
}  // namespace ksa
