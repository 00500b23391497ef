// Kernels of libksa_detect (include/ksa_detect.h): the CFAR row pass, the ordered placement of the emission records and the
// element-wise merge.
//
// row_kernel<VEC, EMIT>: one workgroup of 256 threads owns whole rows, `group` lanes per row (a power of two, 16 .. 256: 256 for
// rows of 1024 bins and more, fewer for shorter rows, which then lie side by side in the workgroup; below 64 a wave holds
// several rows).  Per row:
//   1. Prefix.  The row is read in tiles of group * E adjacent bins (E = 4 with 16-byte loads, 1 with 4-byte loads): a lane
//      quantises its E bins in registers, forms their running sums of q and of `valid`, a scan by __shfl_up over the lanes of a
//      wave that share the row and, where a row spans several waves, the waves' totals through LDS turn them into the row's
//      two exclusive prefix arrays in LDS: int32 P[nbins + 1] and uint16 V[nbins + 1].  A lane stores its E adjacent entries as
//      one 16-byte and one 8-byte store.
//   2. Detection.  Consecutive lanes take consecutive bins, so every LDS access of a wave is to consecutive addresses: a window
//      sum is two reads and a subtraction.  The decisions go into LDS as 64-bit ballot words.  One workgroup-wide OR that is
//      zero (the quiet case) skips everything after it.
//   3. Grouping.  The first wave of the row's lanes walks the ballot words run by run (find-first-set on the words, so a quiet
//      stretch costs one step per 64 bins): runs shorter than min_width are dropped, a kept run at most max_gap bins behind the
//      previous one extends the emission, otherwise it starts the next.
// The pass runs twice.  row_kernel<VEC, false> counts the emissions of every row (and writes the optional floor line);
// sum_kernel / offset_kernel turn the counts into the place of every row's first record, in row order, behind the records the
// buffer already holds; row_kernel<VEC, true> skips the rows without an emission and repeats the others, now with the lanes
// of the walking wave sharing the bins of every kept run (the peak: an integer maximum over q << 32 | ~bin) and of every
// emission (the hits: 64-bit integer atomics), and writes each record as one plain struct store at its place.  No bitmap or
// record crosses global memory between the two, and whatever order the workgroups run in, the buffer is in ascending
// (row, bin_lo) order.
#pragma once
#include <hip/hip_runtime.h>

namespace ksa {
namespace detect {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int SCAN_THREADS = 256;   // rows per workgroup of the offset scan
constexpr int MODE_CA = 0, MODE_GO = 1, MODE_SO = 2;

struct Emission {                   // kse_emission
  long long row;
  int bin_lo, bin_hi, peak_bin, ndet;
  float peak_db, floor_db;
};
static_assert(sizeof(Emission) == 32, "emission record");

// lanes per row: enough for one 16-byte load each up to 1024 bins, never fewer than 16
__host__ __device__ inline int group_for(int nbins) {
  int g = 16;
  while (g < THREADS && g * 4 < nbins) g <<= 1;
  return g;
}

struct Layout {                     // one row's arrays in LDS, in bytes from the row's base
  int v_off, d_off, slot;
};
__host__ __device__ inline Layout layout_for(int nbins) {
  Layout l;
  l.v_off = ((nbins + 1) * 4 + 15) & ~15;
  l.d_off = l.v_off + (((nbins + 1) * 2 + 15) & ~15);
  l.slot = l.d_off + ((((nbins + 63) >> 6) * 8 + 15) & ~15);
  return l;
}

struct RowArgs {
  const float* rows;
  long long row_stride;             // floats
  int* cnt;                         // [nrows] emissions per row: written by the counting pass, read by the emitting pass
  const long long* off;             // [nrows] place of the row's first record (emitting pass)
  float* floor_out;                 // [nrows][nbins] or null (counting pass)
  unsigned long long* hits;         // [nbins]
  Emission* events;                 // [capacity]
  long long row_base;               // running index of row 0 of this launch
  int nrows, nbins, group;
  int train, guard, tq, mode, min_width, max_gap, capacity;
};

__device__ __forceinline__ bool cfar_pass(int q, int s, int c, int tq) { return c > 0 && q * c > s + tq * c; }

__device__ __forceinline__ bool cfar_detect(int mode, int q, int sl, int cl, int sr, int cr, int tq) {
  if (mode == MODE_CA) return cfar_pass(q, sl + sr, cl + cr, tq);
  const bool pl = cfar_pass(q, sl, cl, tq), pr = cfar_pass(q, sr, cr, tq);
  if (mode == MODE_GO) return (cl > 0 || cr > 0) && (cl == 0 || pl) && (cr == 0 || pr);
  return pl || pr;
}

__device__ __forceinline__ float cfar_floor(int s, int c) { return __fdiv_rn((float)s, (float)c) * 0.015625f; }

// first bin at or after p whose ballot bit is `set` (or clear); nbins when there is none
__device__ __forceinline__ int next_bit(const unsigned long long* words, int p, int nbins, bool set) {
  while (p < nbins) {
    unsigned long long w = words[p >> 6];
    if (!set) w = ~w;
    w >>= (p & 63);
    if (w) return min(p + __ffsll((long long)w) - 1, nbins);
    p = (p | 63) + 1;
  }
  return nbins;
}

template <bool VEC, bool EMIT>
__global__ __launch_bounds__(THREADS) void row_kernel(const RowArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ int wave_tot[2][2][WAVES];                 // [buffer][sum of q | count][wave]
  constexpr int E = VEC ? 4 : 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nbins = a.nbins, G = a.group, W = min(G, 64);
  const int slot = tid / G, gl = tid & (G - 1), rpw = THREADS / G;
  const int nwords = (nbins + 63) >> 6;
  const Layout lay = layout_for(nbins);
  int* P = reinterpret_cast<int*>(lds + slot * lay.slot);
  unsigned short* V = reinterpret_cast<unsigned short*>(lds + slot * lay.slot + lay.v_off);
  unsigned long long* D = reinterpret_cast<unsigned long long*>(lds + slot * lay.slot + lay.d_off);
  const int ntiles = (nbins + G * E - 1) / (G * E);
  const int npasses = (a.nrows + rpw - 1) / rpw;

  for (int pass = blockIdx.x; pass < npasses; pass += gridDim.x) {        // every trip count below is workgroup-uniform
    const int r = pass * rpw + slot;
    const bool rok = r < a.nrows;
    if constexpr (EMIT) {
      const int c = rok ? a.cnt[r] : 0;
      if (!__syncthreads_or(c > 0)) continue;
    }
    const float* row = a.rows + (long long)(rok ? r : 0) * a.row_stride;

    // 1. the two exclusive prefix arrays
    int carry_s = 0, carry_c = 0, buf = 0;              // a pass carries nothing over from the one before
    for (int t = 0; t < ntiles; ++t) {
      const int b0 = (t * G + gl) * E;
      const bool ok = rok && b0 < nbins;
      float x[E];
#pragma unroll
      for (int j = 0; j < E; ++j) x[j] = 0.0f;
      if (ok) {
        if constexpr (VEC) {
          const float4 v = *reinterpret_cast<const float4*>(row + b0);
          x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
        } else {
          x[0] = row[b0];
        }
      }
      int ex_s[E], ex_c[E], ls = 0, lc = 0;
#pragma unroll
      for (int j = 0; j < E; ++j) {
        const bool valid = ok && !(x[j] != x[j]) && x[j] != -INFINITY;
        const int q = valid ? (int)rintf(fminf(fmaxf(x[j], -500.0f), 500.0f) * 64.0f) : 0;
        ex_s[j] = ls;
        ex_c[j] = lc;
        ls += q;
        lc += valid ? 1 : 0;
      }
      int is = ls, ic = lc;                             // inclusive over the lanes of this wave that share the row
      for (int d = 1; d < W; d <<= 1) {
        const int ts = __shfl_up(is, d, W), tc = __shfl_up(ic, d, W);
        if ((lane & (W - 1)) >= d) {
          is += ts;
          ic += tc;
        }
      }
      int before_s = 0, before_c = 0, tot_s, tot_c;
      if (G > 64) {                                     // the row spans G / 64 waves
        if (lane == 63) {
          wave_tot[buf][0][wave] = is;
          wave_tot[buf][1][wave] = ic;
        }
        __syncthreads();
        const int first = wave & ~(G / 64 - 1);
        tot_s = tot_c = 0;
        for (int w = 0; w < G / 64; ++w) {
          const int s = wave_tot[buf][0][first + w], c = wave_tot[buf][1][first + w];
          if (first + w < wave) {
            before_s += s;
            before_c += c;
          }
          tot_s += s;
          tot_c += c;
        }
        buf ^= 1;                                       // the next tile writes the other buffer: one barrier per tile
      } else {
        tot_s = __shfl(is, W - 1, W);
        tot_c = __shfl(ic, W - 1, W);
      }
      const int base_s = carry_s + before_s + is - ls, base_c = carry_c + before_c + ic - lc;
      if (ok) {
        if constexpr (VEC) {
          *reinterpret_cast<int4*>(P + b0) = make_int4(base_s + ex_s[0], base_s + ex_s[1], base_s + ex_s[2], base_s + ex_s[3]);
          *reinterpret_cast<ushort4*>(V + b0) = make_ushort4((unsigned short)(base_c + ex_c[0]), (unsigned short)(base_c + ex_c[1]),
                                                              (unsigned short)(base_c + ex_c[2]), (unsigned short)(base_c + ex_c[3]));
        } else {
          P[b0] = base_s;
          V[b0] = (unsigned short)base_c;
        }
      }
      carry_s += tot_s;
      carry_c += tot_c;
    }
    if (gl == 0) {
      P[nbins] = carry_s;
      V[nbins] = (unsigned short)carry_c;
    }
    __syncthreads();

    // 2. detection: consecutive lanes, consecutive bins; 64-bit ballot words into LDS
    bool any = false;
    unsigned long long acc0 = 0, acc1 = 0;              // G < 64: a row has at most two words, gathered in registers
    const int span = G >= 64 ? nwords * 64 : nbins;
    for (int base = 0; base < span; base += G) {
      const int b = base + gl;
      bool det = false;
      if (rok && b < nbins) {
        const int i0 = max(b - a.guard - a.train, 0), i1 = max(b - a.guard, 0);
        const int i2 = min(b + a.guard + 1, nbins), i3 = min(b + a.guard + 1 + a.train, nbins);
        const int sl = P[i1] - P[i0], cl = (int)V[i1] - (int)V[i0];
        const int sr = P[i3] - P[i2], cr = (int)V[i3] - (int)V[i2];
        const int q = P[b + 1] - P[b];
        const bool valid = V[b + 1] != V[b];
        det = valid && cfar_detect(a.mode, q, sl, cl, sr, cr, a.tq);
        if constexpr (!EMIT) {
          if (a.floor_out) a.floor_out[(long long)r * nbins + b] = cfar_floor(sl + sr, cl + cr);
        }
      }
      const unsigned long long votes = __ballot(det);
      any = any || votes != 0ull;
      if (G >= 64) {
        const int word = b >> 6;                        // wave-uniform: b - lane is a multiple of 64
        if (lane == 0 && word < nwords) D[word] = votes;
      } else {
        const unsigned long long part = (votes >> (lane & ~(G - 1))) & ((1ull << G) - 1ull);
        if (base < 64) acc0 |= part << base;
        else acc1 |= part << (base - 64);
      }
    }
    if (G < 64 && gl == 0) {
      D[0] = acc0;
      if (nwords > 1) D[1] = acc1;
    }
    if (!__syncthreads_or(any)) {                       // the quiet case: nothing was detected in any row of this pass
      if constexpr (!EMIT) {
        if (gl == 0 && rok) a.cnt[r] = 0;
      }
      continue;
    }

    // 3. grouping: the first wave of the row's lanes walks the runs
    int count = 0;
    if (gl < W && rok) {
      long long best = 0;
      int lo = 0, hi = 0, ndet = 0;
      long long place = 0;
      if constexpr (EMIT) place = a.off[r];
      auto close = [&]() {
        if constexpr (EMIT) {
          for (int m = 1; m < W; m <<= 1) {
            const long long other = __shfl_xor(best, m, W);
            best = other > best ? other : best;
          }
          for (int b = lo + gl; b <= hi; b += W) atomicAdd(&a.hits[b], 1ull);
          const long long pos = place + (count - 1);
          if (gl == 0 && pos < (long long)a.capacity) {
            const int pk = (int)(0x7FFFFFFFu - (unsigned)(best & 0xFFFFFFFFll));
            const int i0 = max(pk - a.guard - a.train, 0), i1 = max(pk - a.guard, 0);
            const int i2 = min(pk + a.guard + 1, nbins), i3 = min(pk + a.guard + 1 + a.train, nbins);
            const int sl = P[i1] - P[i0], cl = (int)V[i1] - (int)V[i0];
            const int sr = P[i3] - P[i2], cr = (int)V[i3] - (int)V[i2];
            int s = sl + sr, c = cl + cr;
            if (a.mode != MODE_CA) {
              const long long l = (long long)sl * cr, rr = (long long)sr * cl;      // mean_l against mean_r, no division
              const bool lag = cr == 0 || (cl > 0 && (a.mode == MODE_GO ? l >= rr : l <= rr));
              s = lag ? sl : sr;
              c = lag ? cl : cr;
            }
            Emission e;
            e.row = a.row_base + r;
            e.bin_lo = lo;
            e.bin_hi = hi;
            e.peak_bin = pk;
            e.ndet = ndet;
            e.peak_db = row[pk];
            e.floor_db = cfar_floor(s, c);
            a.events[pos] = e;
          }
        }
      };
      bool open = false;
      int p = 0;
      while (true) {
        const int s = next_bit(D, p, nbins, true);
        if (s >= nbins) break;
        const int e = next_bit(D, s, nbins, false);     // one past the run
        p = e;
        if (e - s < a.min_width) continue;
        if (!open || s - hi - 1 > a.max_gap) {
          if (open) close();
          open = true;
          ++count;
          lo = s;
          ndet = 0;
          best = 0;
        }
        hi = e - 1;
        ndet += e - s;
        if constexpr (EMIT) {
          for (int b = s + gl; b < e; b += W) {
            const long long key = ((long long)(P[b + 1] - P[b] + 65536) << 32) | (long long)(0x7FFFFFFFu - (unsigned)b);
            best = key > best ? key : best;
          }
        }
      }
      if (open) close();
    }
    if constexpr (!EMIT) {
      if (gl == 0 && rok) a.cnt[r] = count;
    }
    __syncthreads();                                    // the walk reads what the next pass overwrites
  }
}

struct ScanArgs {
  const int* cnt;                   // [nrows]
  int nrows;
  int* row_count;                   // [nrows] or null: the caller's copy of cnt
  long long* block_sums;            // [ceil(nrows / SCAN_THREADS)]
  long long* total;                 // emissions_total
  long long* snapshot;              // emissions_total as it was before this launch
  long long* off;                   // [nrows]
};

__global__ __launch_bounds__(SCAN_THREADS) void sum_kernel(const ScanArgs a) {
  __shared__ long long part[SCAN_THREADS / 64];
  const int tid = threadIdx.x, i = blockIdx.x * SCAN_THREADS + tid;
  const int c = i < a.nrows ? a.cnt[i] : 0;
  if (a.row_count && i < a.nrows) a.row_count[i] = c;
  long long s = c;
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
  const int c = i < a.nrows ? a.cnt[i] : 0;
  int inc = c;                                          // at most 256 rows of at most 8192 emissions
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
  if (i < a.nrows) a.off[i] = pos + mine;
  if (blockIdx.x == gridDim.x - 1 && tid == 0) *a.total = pos + all;
}

__global__ void merge_kernel(long long* hits, const long long* other, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    hits[i] += other[i];
}

}  // namespace detect
}  // namespace ksa
