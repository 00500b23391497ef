// libksa: C ABI (include/ksa.h) over the gfx950 kernels in ksa_kernels.hpp.
// Host-side orchestration only: table generation, scratch, launches, state hand-off.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/ksa.h"
#include "ksa_dif16.hpp"
#include "ksa_kernels.hpp"
#include "ksa_kernels32.hpp"
#include "ksa_kernels64.hpp"
#include "ksa_kernels_pair.hpp"
#include "ksa_kernels_mr.hpp"
#include "ksa_pfb.hpp"
#include "ksa_tables.hpp"

namespace {

thread_local std::string g_err;

int fail(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return 1;
}

#define HIP_OK(call)                                                                      \
  do {                                                                                    \
    hipError_t _e = (call);                                                               \
    if (_e != hipSuccess) return fail("%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)

bool is_pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }

// fft_size of the mixed-radix path (6): 2^a * 3^b * 5^c, a multiple of 4 (float4 rows), 16 .. 16384 (one transform in LDS),
// not a power of two (those keep their own plans)
bool is_mixed_radix(int n) {
  if (n < 16 || n > 16384 || n % 4 || is_pow2(n)) return false;
  int m = n;
  for (int f : {2, 3, 5})
    while (m % f == 0) m /= f;
  return m == 1;
}

// Entry points run on their engine's device and hand the caller's current device back on every exit path (a process that
// drives one engine per GPU, or torch beside libksa, keeps its own notion of "current").
struct DeviceGuard {
  int prev = -1;
  DeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// A/B switches of the measurement builds (tools/variants.sh compiles with -DKSA_EXPERIMENTS).  The shipped library reads
// no environment variable: which kernel a user runs depends on the engine's configuration only.
#ifdef KSA_EXPERIMENTS
const char* exp_env(const char* name) { return getenv(name); }
#else
constexpr const char* exp_env(const char*) { return nullptr; }
#endif

// default first-stage scratch per chunk of frames (ksa_dif16.hpp); tuned on MI355X, see DESIGN.md 4.2
#ifndef KSA_DIF_SCRATCH_MB_DEFAULT
#define KSA_DIF_SCRATCH_MB_DEFAULT 4096
#endif

// KSA_CUMU_PFB: bytes of folded frames (complex64 [frames][N]) that one fold + transform chunk holds in engine scratch: the
// bound of that scratch.  Measured at 16 / 64 / 256 MiB (profiles/pfb_sweep.txt): the larger the faster -- every chunk is a fold
// launch and a transform launch that drain one after the other, which keeping a chunk inside the last-level cache does not
// pay back.
#ifndef KSA_PFB_CHUNK_BYTES
#define KSA_PFB_CHUNK_BYTES (256ll << 20)
#endif

}  // namespace

struct ksa_engine {
  ksa_config cfg{};
  hipStream_t stream = nullptr;
  int num_cu = 0;
  // tables
  int* d_starts = nullptr;
  int* d_start_last = nullptr;  // RAW mode: the last window only
  float* d_window = nullptr;
  float* d_window32 = nullptr;  // 32-point plan: the same taps as [8][N/32][4] (16-byte tap loads, ksa_kernels32.hpp)
  float2* d_tw_mid = nullptr;
  float2* d_tw_last = nullptr;
  float* d_adj = nullptr;       // zeroSpan Fft.Adj or null
  float* d_scan_adj = nullptr;
  // scratch
  void* d_iq_stage = nullptr;   // one block for the host-pointer entry points
  float* d_frames = nullptr;    // [max_frames][N] per-frame spectra when the caller passes none
  float* d_part = nullptr;      // [chunks][3][N]
  float* d_xchg = nullptr;      // one block [4][N] partial | [128][hm_width] ring: what a rank sends to the others
  float* d_partial = nullptr;   // [4][N]            (= d_xchg)
  float* d_state = nullptr;     // [4][N] cur,max,min,avg
  float* d_hm = nullptr;        // [128][hm_width]   (= d_xchg + 4N)
  float* d_scan_state = nullptr;  // [4][total]
  float* d_scan_hm = nullptr;     // [128][scan_hm_width]
  float* d_scan_avg_rows = nullptr;  // [128][total] Fft.Avg after each of a batch's last passes (multi-pass stitch)
  float* d_levels = nullptr;      // [4][cells] plot-side decimation scratch
  int* d_highs = nullptr;         // peak markers: [HIGHS_MAX] cell | [HIGHS_MAX] level (float bits) | found
  float* d_parts = nullptr;       // [capacity][N] partial folds of the window-split (latency) mode
  unsigned* d_tickets = nullptr;  // the unit counter of spectrum_kernel's ticket walk: this engine's alone, zeroed on its stream before every launch
  int levels_cap = 0;
  // multi-engine merges inside one process (ksa_allreduce_state, ksa_scan_allstitch) and the host-pointer scan pass
  float* d_gather = nullptr;      // [n][4N + 128W] every engine's exchange block, or [n][rows][scan_hm_width]
  size_t gather_cap = 0;          // floats
  void* d_scan_stage = nullptr;   // [nsteps][full_size] capture blocks of ksa_scan_pass_c64 / _u8
  size_t scan_stage_cap = 0;      // bytes
  float* d_scan_rows = nullptr;   // [128][scan_hm_width] partial waterfall rows of a band-sharded batch
  int scan_rows = 0;              // rows the last ksa_scan_stitch_range_dev wrote
  int scan_rows_passes = 0;       // ... and the passes of that batch (ring advance of ksa_scan_merge_rows_dev)
  float* d_scan_halo = nullptr;   // [nhalo][npasses][N] halo bands (ksa_scan_allstitch)
  float* d_scan_send = nullptr;   // [nhalo][npasses][N] own bands packed for the right neighbours
  size_t scan_halo_cap = 0, scan_send_cap = 0;   // floats
  hipEvent_t ev_ready = nullptr, ev_copied = nullptr, ev_stream = nullptr;
  // zeroSpan batches from host memory (ksa_frames_c64 / _u8): capture blocks cross PCIe slot by slot on copy_stream
  hipStream_t copy_stream = nullptr;               // engine-owned, created on first use
  void* d_slot[2] = {nullptr, nullptr};            // [slot frames][full_size] samples each
  size_t slot_cap[2] = {0, 0};                     // bytes
  hipEvent_t ev_slot_copied[2] = {nullptr, nullptr}, ev_slot_read[2] = {nullptr, nullptr}, ev_copy_start = nullptr;
  float* d_host_rows = nullptr;                    // [nframes][hm_width] waterfall rows a host caller asked for
  size_t host_rows_cap = 0;                        // floats
  int plan_frames = 0;          // the spectrum launch in flight picks its shape for this many frames (>= its own nframes)
  // N > 16384: radix-16 / 32 / 64 decimation in frequency in front of the single-workgroup kernel (ksa_dif16.hpp)
  int sub_n = 0;                // size of the single-workgroup transform: fft_size (path 0) or fft_size/16 (path 2)
  float2* d_dif_tw = nullptr;   // [6][N1]
  float2* d_dif_z = nullptr;    // [chunk][16][nwin][N1]
  float* d_dif_y = nullptr;     // [chunk][16][N1]
  float* d_ones = nullptr;      // [N1] taps of the second stage (the window was applied in the first)
  int* d_starts_b = nullptr;    // [nwin] w*N1
  int dif_chunk = 1;
  int dif_radix = 16;           // first-stage radix: 16 (N <= 262144), 32 (524288), 64 (1048576)
  // KSA_CUMU_PFB (ksa_pfb.hpp): the fold's tables and its output.  d_starts / d_window then hold the transform stage's inner
  // shape (one window at 0, all-ones taps); cfg keeps the caller's outer shape (full_size, num_windows = taps).
  int* d_pfb_starts = nullptr;  // [P] the caller's window_starts
  float* d_pfb_taps = nullptr;  // [P][N] the caller's window
  float2* d_pfb_y = nullptr;    // [pfb_chunk][N] folded frames
  int pfb_chunk = 0;            // frames per fold + transform chunk (a multiple of 4)
  bool pfb_ring_ok = false;     // starts[k] == k*N and P in {4, 8, 16}: the ring kernel may serve frame_stride == N
  // KSA_CUMU_PFB_PSD: every block folds into pfb_sub (K) sub-frames, d_pfb_y is [pfb_chunk][K][N] and the inner shape K
  // rectangular windows at j*N over a folded frame of K*N samples (1 on a KSA_CUMU_PFB engine: one folded frame per block)
  int pfb_sub = 1;
  // bookkeeping
  long long frames_seen = 0;
  int hm_index = 0;
  int pending_frames = 0;       // frames of the last uncommitted batch
  int b_max = 1, b_min = 1, b_avg = 1;
  int has_max = 0, has_min = 0, has_avg = 0;   // the curve holds frames already (seeded by copy otherwise, K:133-134)
  int scan_base_is_raw = 0;
  long long scan_passes = 0;
  int scan_hm_index = 0;
  int max_chunks = 1;
  // launch config of the spectrum kernel
  int path = 0, threads = 0, lds_bytes = 0, vgprs = 0, blocks_per_cu = 1;
  int reuse_m = 0;              // new samples per thread per window when hops are a fixed multiple of N/16
  bool plan32 = false;          // 8192 / 16384: the 32-points-per-thread kernel (ksa_kernels32.hpp)
  // 1024 .. 4096, large batches: two frames per workgroup in packed fp32 (ksa_kernels_pair.hpp)
  bool pair_ok = false;
  int pair_bpc = 0, pair_vgprs = 0, pair_lds = 0;
  // N = 64, complex64: the 8 x 8 plan with adjacent-sample loads (ksa_kernels64.hpp)
  bool k64_ok = false;
  bool win_ones = false;          // every tap of the window table is exactly 1.0f (the reference's default window, K:52)
  int k64_bpc = 0, k64_vgprs = 0;
  // path 6: fft_size 2^a * 3^b * 5^c (ksa_kernels_mr.hpp); the plan's twiddles live in d_tw_mid
  ksa::MrPlan mr{};
  // profiling
  bool prof = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
  double prof_ms = 0;
  long long prof_launches = 0;
  // clock stamps around profiled spectrum stages (ksa_prof_clock, ksa::clock_stamp_kernel)
  unsigned long long* d_clk = nullptr;      // [CLK_SLOTS][before | after][CLK_KEYS][memtime, memrealtime]
  long long clk_launches = 0;
};

namespace {

using ksa::SpecParams;

// The frame count a launch chooses its shape for (pair kernel, window split and its parts): the launch's own, or that of the
// whole batch when a host batch arrives slot by slot (ksa_frames_c64 / _u8) -- every slot then gets the whole batch's plan.
int plan_of(const ksa_engine* e, const SpecParams& p) { return std::max(p.nframes, e->plan_frames); }

// KSA_CUMU_PSD engines run the CUMU_PSD instantiation of every spectrum kernel (a template constant everywhere, also where the
// other folds branch at run time) with SpecParams::cumu = CUMU_AVG: the combines and the output stage of the two are the same.
// A KSA_CUMU_PFB_PSD engine's transform stage is that of a KSA_CUMU_PSD engine of K rectangular windows at hop N on complex64.
bool fold_psd(const ksa_engine* e) { return e->cfg.cumu_mode == KSA_CUMU_PSD || e->cfg.cumu_mode == KSA_CUMU_PFB_PSD; }
// KSA_CUMU_PFB engines fold in the time domain (ksa_pfb.hpp) and run the AVG instantiations on one window per folded frame.
bool fold_pfb(const ksa_engine* e) { return e->cfg.cumu_mode == KSA_CUMU_PFB; }
// KSA_CUMU_PFB_PSD engines fold every block into K sub-frames in the time domain and run the PSD instantiations over them.
bool fold_pfb_psd(const ksa_engine* e) { return e->cfg.cumu_mode == KSA_CUMU_PFB_PSD; }
// either of the two: a fold stage in front of the transform stage
bool fold_time(const ksa_engine* e) { return fold_pfb(e) || fold_pfb_psd(e); }
// bytes per IQ sample of a KSA_FMT_* value
size_t sample_bytes(int fmt) { return fmt == KSA_FMT_C64 ? 8 : fmt == KSA_FMT_S16 ? 4 : 2; }

// ---- run-time value -> template constant, each choice written once ---------------------------------------------------------
template <int V>
using int_c = std::integral_constant<int, V>;
template <int... V>
struct Ints {};

// f(int_c<V>{}) for the V of the list that equals `value`; -1 when the list does not hold it (f returns 0 or 1).
template <class F, int... V>
int dispatch(int value, Ints<V...>, F&& f) {
  int rc = -1;
  (void)((value == V && ((rc = f(int_c<V>{})), true)) || ...);
  return rc;
}

// Every sample format, complex64 first: what with_fmt dispatches over and what the configure pass of ksa_create walks.
// (include/ksa.h and the kernels number the formats alike.)
using Formats = Ints<ksa::FMT_C64, ksa::FMT_U8, ksa::FMT_S8, ksa::FMT_S16>;
static_assert(KSA_FMT_C64 == ksa::FMT_C64 && KSA_FMT_U8 == ksa::FMT_U8 && KSA_FMT_S8 == ksa::FMT_S8 && KSA_FMT_S16 == ksa::FMT_S16, "");

template <class F>
int with_fmt(int fmt, F&& f) {
  const int rc = dispatch(fmt, Formats{}, f);
  return rc < 0 ? fail("unknown sample format %d", fmt) : rc;
}
template <class F, int... FMT>
int for_each_fmt(Ints<FMT...>, F&& f) {
  int rc = 0;
  (void)((rc = f(int_c<FMT>{})) || ...);
  return rc;
}

// Sizes of the 16-point single-workgroup plan (ksa::Plan<N>).
#ifdef KSA_EXPERIMENTS   // the 16-point plan at 8192 / 16384 is reachable through KSA_PLAN16 only
using Sizes = Ints<16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384>;
#else
using Sizes = Ints<16, 32, 64, 128, 256, 512, 1024, 2048, 4096>;
#endif
template <class F>
int with_size(int sub_n, F&& f) {
  const int rc = dispatch(sub_n, Sizes{}, f);
  return rc < 0 ? fail("fft_size %d has no single-workgroup plan", sub_n) : rc;
}

using Radices = Ints<16, 32, 64>;   // first stage of N > 16384 (ksa_engine::dif_radix)

// Fold mode as a template constant.  A KSA_CUMU_PSD engine: CUMU_PSD.  Otherwise the configure pass visits MAX, MIN, then AVG
// (AVG last, so that the attributes a launcher records describe the AVG instantiation) and a launch the mode p.cumu names.
template <class F>
int with_fold(const ksa_engine* e, const SpecParams& p, bool cfg_only, F&& f) {
  if (fold_psd(e)) return f(int_c<ksa::CUMU_PSD>{});
  if (cfg_only) {
    if (f(int_c<ksa::CUMU_MAX>{}) || f(int_c<ksa::CUMU_MIN>{})) return 1;
    return f(int_c<ksa::CUMU_AVG>{});
  }
  if (p.cumu == ksa::CUMU_AVG) return f(int_c<ksa::CUMU_AVG>{});
  if (p.cumu == ksa::CUMU_MAX) return f(int_c<ksa::CUMU_MAX>{});
  return f(int_c<ksa::CUMU_MIN>{});
}
constexpr bool fold_avg_or_psd(int cm) { return cm == ksa::CUMU_AVG || cm == ksa::CUMU_PSD; }

// Configure pass of one kernel instantiation: allow it `lds_attr` bytes of dynamic LDS (default: what it is launched with) and
// report its registers and its workgroups per CU at `threads` x `lds_bytes`.  Whether that goes into the engine is the caller's.
struct KernelFit {
  int vgprs = 0, blocks_per_cu = 1;
};
template <class K>
int configure_kernel(K kfn, int threads, int lds_bytes, KernelFit* fit, int lds_attr = -1) {
  HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, lds_attr < 0 ? lds_bytes : lds_attr));
  hipFuncAttributes attr;
  HIP_OK(hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(kfn)));
  int occ = 0;
  HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kfn, threads, lds_bytes));
  fit->vgprs = attr.numRegs;
  fit->blocks_per_cu = std::max(1, occ);
  return 0;
}

// Launch of a persistent n-point spectrum kernel over a batch.  Small batches (the per-frame drop-in, one scan pass) where
// `may_split`: every frame's windows are split over several workgroups so that the GPU is filled, and the partial folds are
// combined by a second, tiny kernel (pays from N = 1024 up: 84 -> 51 us per block at N=4096, 720 -> 117 us at N=16384; tiny
// transforms only lose the launches).  `grid_cap` bounds the grid (measurements; INT_MAX otherwise).
// `tickets` (spectrum_kernel at one transform per workgroup): units are handed out on demand through the engine's counter, which is
// zeroed on the stream in front of the launch (launches of one engine are stream-ordered: one counter serves them all).  Only
// where a unit is long enough that the draws stay rare -- one atomic per unit on one address: a unit of TICKET_MIN_POINTS
// window points is some 20 us of a workgroup (4 us per 4096-point window at three workgroups per CU); shorter units (RAW mode,
// few windows at N = 1024, thin window-split shares) keep the static walk, as do the kernels of several transforms per workgroup.
constexpr long long TICKET_MIN_POINTS = 5 * 4096;
template <class K>
int launch_split(ksa_engine* e, K kfn, const SpecParams& p, int n, int threads, int lds_bytes, bool may_split, int grid_cap, bool tickets = false) {
  const int capacity = e->num_cu * e->blocks_per_cu;
  SpecParams q = p;
  const int plan = plan_of(e, p);
  if (e->d_parts && may_split && !exp_env("KSA_NO_SPLIT") && p.nwin > 1 && plan * 2 <= capacity) {
    q.parts = std::min(p.nwin, capacity / plan);
    q.part_out = e->d_parts;
  }
  int grid = std::max(1, std::min(q.nframes * std::max(1, q.parts), capacity));
  grid = std::max(1, std::min(grid, grid_cap));
  if (tickets && e->d_tickets && !exp_env("KSA_STATIC_WALK") && (long long)(p.nwin / std::max(1, q.parts)) * n >= TICKET_MIN_POINTS) {
    HIP_OK(hipMemsetAsync(e->d_tickets, 0, sizeof(unsigned), e->stream));
    q.tickets = e->d_tickets;
  }
  hipLaunchKernelGGL(kfn, dim3(grid), dim3(threads), lds_bytes, e->stream, q);
  if (q.parts > 1) {
    hipLaunchKernelGGL(ksa::combine_parts_kernel, dim3((n / 4 + 63) / 64, q.nframes), dim3(64), 0, e->stream, q, n);
    if (q.hm_w > 0)
      hipLaunchKernelGGL(ksa::rowmax_batch, dim3((q.hm_w + 255) / 256, q.nframes), dim3(256), 0, e->stream, q, n);
  }
  HIP_OK(hipGetLastError());
  return 0;
}

// The same walk for spectrum64_kernel / spectrum_pair_kernel (`units` frames / pairs of `points` window points each, at most `cap`
// workgroups): their units are short, so a ticket covers a run of consecutive units that holds >= TICKET_MIN_POINTS points, and only
// batches in which every workgroup draws at least two runs take it -- smaller ones keep the stride walk and the grid they had.
// Sets q.tickets / q.ticket_run (zeroing the counter on the stream) and returns the grid; < 0 on a HIP error.
int ticket_runs(ksa_engine* e, SpecParams& q, int units, long long points, int cap) {
  if (const char* g = exp_env("KSA_GRID")) cap = std::max(1, std::min(cap, atoi(g)));
  const int run = (int)std::max<long long>(1, (TICKET_MIN_POINTS + points - 1) / std::max<long long>(1, points));
  q.ticket_run = 1;
  if (e->d_tickets && !exp_env("KSA_STATIC_WALK") && units >= 2ll * cap * run) {
    if (hipMemsetAsync(e->d_tickets, 0, sizeof(unsigned), e->stream) != hipSuccess) return -1;
    q.tickets = e->d_tickets;
    q.ticket_run = run;
    return cap;
  }
  return std::max(1, std::min(units, cap));
}

template <int N, int FMT, int RM, int CM>
int launch_pair_c(ksa_engine* e, const SpecParams& p, bool configure_only) {
  using PP = ksa::PlanPair<N>;
  auto kfn = ksa::spectrum_pair_kernel<N, FMT, RM, CM>;
  if (configure_only) {
    KernelFit fit;
    if (configure_kernel(kfn, ksa::Plan<N>::T, PP::LDS_BYTES, &fit)) return 1;
    if (FMT == ksa::FMT_C64 && fold_avg_or_psd(CM)) {
      e->pair_bpc = fit.blocks_per_cu;
      e->pair_vgprs = fit.vgprs;
      e->pair_lds = PP::LDS_BYTES;
    }
    return 0;
  }
  const int npairs = (p.nframes + 1) / 2;
  SpecParams q = p;
  const int grid = ticket_runs(e, q, npairs, 2ll * p.nwin * N, e->num_cu * e->pair_bpc);
  if (grid < 0) return fail("hipMemsetAsync of the ticket counter failed");
  hipLaunchKernelGGL(kfn, dim3(grid), dim3(ksa::Plan<N>::T), PP::LDS_BYTES, e->stream, q);
  HIP_OK(hipGetLastError());
  return 0;
}

template <int N, int FMT, int RM>
int launch_pair(ksa_engine* e, const SpecParams& p, bool cfg_only) {
  return with_fold(e, p, cfg_only, [&](auto cm) { return launch_pair_c<N, FMT, RM, decltype(cm)::value>(e, p, cfg_only); });
}

template <int N, int FMT, int RM, int CM>
int launch_spec_c(ksa_engine* e, const SpecParams& p, bool configure_only) {
  using P = ksa::Plan<N>;
  auto kfn = ksa::spectrum_kernel<N, FMT, RM, CM>;
#ifdef KSA_EXPERIMENTS
  // KSA_PLAIN: the plain-arithmetic instantiation of a kernel that ships with packed butterflies (Tune<N>::packed)
  if constexpr (ksa::Tune<N>::packed(RM)) {
    if (exp_env("KSA_PLAIN")) kfn = ksa::spectrum_plain_kernel<N, FMT, RM, CM>;
  }
#endif
  static const int lds_pad = exp_env("KSA_LDS_PAD_KB") ? atoi(exp_env("KSA_LDS_PAD_KB")) * 1024 : 0;   // occupancy experiments
  const int lds_bytes = ksa::Tune<N>::LDS_BYTES + lds_pad;
  if (configure_only) {
    KernelFit fit;
    if (configure_kernel(kfn, P::T, lds_bytes, &fit)) return 1;
    if (FMT == ksa::FMT_C64) {      // (whatever the fold constant: the last one configured stands)
      e->threads = P::T;
      e->lds_bytes = ksa::Tune<N>::LDS_BYTES;
      e->vgprs = fit.vgprs;
      e->blocks_per_cu = fit.blocks_per_cu;
    }
    return 0;
  }
  const char* g = exp_env("KSA_GRID");   // measurement: fewer persistent workgroups
  return launch_split(e, kfn, p, N, P::T, lds_bytes, N >= 1024, g ? atoi(g) : INT_MAX, P::S == 1);
}

template <int N, int FMT, int RM>
int launch_spec_t(ksa_engine* e, const SpecParams& p, bool configure_only) {
  // large batches of 1024 .. 4096-point transforms: two frames per workgroup in packed fp32
#ifdef KSA_EXPERIMENTS
  constexpr bool pair_size = ksa::Plan<N>::S == 1 && ksa::Plan<N>::T <= 256 && ksa::Plan<N>::M >= 2;   // 1024 .. 4096 (KSA_PAIR_ALL)
#else
  constexpr bool pair_size = N == 1024;     // where it measured faster: the only size the product instantiates
#endif
  if constexpr (pair_size) {
    if (e->pair_ok) {
      if (configure_only) {
        // every reuse variant a later batch can pick (RAW mode runs RM = 0 whatever the hops); the one in use last,
        // so that pair_bpc / pair_vgprs describe it
        if (RM != 0 && launch_pair<N, FMT, 0>(e, p, true)) return 1;
        if (RM != 4 && launch_pair<N, FMT, 4>(e, p, true)) return 1;
        if (RM != 8 && launch_pair<N, FMT, 8>(e, p, true)) return 1;
        if (launch_pair<N, FMT, RM>(e, p, true)) return 1;
      } else if (plan_of(e, p) >= 2 * e->num_cu * e->pair_bpc) return launch_pair<N, FMT, RM>(e, p, false);
    }
  }
  // fold mode as a template constant (Tune<N>::fold_const) or as a run-time branch inside the window loop
  if constexpr (ksa::Tune<N>::fold_const(RM)) {
    return with_fold(e, p, configure_only, [&](auto cm) { return launch_spec_c<N, FMT, RM, decltype(cm)::value>(e, p, configure_only); });
  } else {
    if (fold_psd(e)) return launch_spec_c<N, FMT, RM, ksa::CUMU_PSD>(e, p, configure_only);
    return launch_spec_c<N, FMT, RM, 0>(e, p, configure_only);
  }
}

// sample-reuse variants exist where one transform fills the workgroup and the carried samples fit the register
// budget (N = 1024..4096).  At T >= 512 (128-VGPR cap) the carried registers spill: measured 9..28 % slower than
// re-reading the overlap through L2 (N=8192: 42.6 vs 46.3 M FFT/s at 50 %, 40.7 vs 51.9 at 75 %; N=16384: 20.4 vs
// 23.3 and 19.7 vs 25.0), so those sizes take the general path.
template <int N, int FMT>
int launch_spec_rm(ksa_engine* e, const SpecParams& p, bool cfg_only, int rm) {
  if constexpr (ksa::Plan<N>::S == 1 && ksa::Plan<N>::T <= 256) {
    if (rm == 8) return launch_spec_t<N, FMT, 8>(e, p, cfg_only);
    if (rm == 4) return launch_spec_t<N, FMT, 4>(e, p, cfg_only);
  }
  return launch_spec_t<N, FMT, 0>(e, p, cfg_only);
}

// 32 points per thread (N = 8192, 16384): fold mode always a template constant
template <int N, int FMT, int CM>
int launch_spec32_c(ksa_engine* e, const SpecParams& p, bool configure_only) {
  using P = ksa::Plan32<N>;
  auto kfn = ksa::spectrum32_kernel<N, FMT, CM>;
  if (configure_only) {
    KernelFit fit;
    if (configure_kernel(kfn, P::T, P::LDS_BYTES, &fit)) return 1;
    if (FMT == ksa::FMT_C64 && fold_avg_or_psd(CM)) {
      e->threads = P::T;
      e->lds_bytes = P::LDS_BYTES;
      e->vgprs = fit.vgprs;
      e->blocks_per_cu = fit.blocks_per_cu;
    }
    return 0;
  }
  const char* g = exp_env("KSA_GRID");   // measurement: fewer persistent workgroups
  return launch_split(e, kfn, p, N, P::T, P::LDS_BYTES, true, g ? atoi(g) : INT_MAX);
}

template <int N, int FMT>
int launch_spec32(ksa_engine* e, const SpecParams& p, bool cfg_only) {
  return with_fold(e, p, cfg_only, [&](auto cm) { return launch_spec32_c<N, FMT, decltype(cm)::value>(e, p, cfg_only); });
}

// N = 64, complex64 input: 8 x 8 with adjacent samples per lane (ksa_kernels64.hpp)
template <int CM, bool W1>
int launch_spec64_c(ksa_engine* e, const SpecParams& p, bool configure_only) {
  auto kfn = ksa::spectrum64_kernel<ksa::FMT_C64, CM, W1>;
  if (configure_only) {
    KernelFit fit;
    if (configure_kernel(kfn, ksa::Plan64::T, ksa::Plan64::LDS_BYTES, &fit)) return 1;
    if (fold_avg_or_psd(CM)) {
      e->k64_bpc = fit.blocks_per_cu;
      e->k64_vgprs = fit.vgprs;
    }
    return 0;
  }
  SpecParams q = p;
  const int grid = ticket_runs(e, q, p.nframes, (long long)p.nwin * ksa::Plan64::N, e->num_cu * e->k64_bpc);
  if (grid < 0) return fail("hipMemsetAsync of the ticket counter failed");
  hipLaunchKernelGGL(kfn, dim3(grid), dim3(ksa::Plan64::T), ksa::Plan64::LDS_BYTES, e->stream, q);
  HIP_OK(hipGetLastError());
  return 0;
}

int launch_spec64(ksa_engine* e, const SpecParams& p, bool cfg_only) {
  // (p.window is the engine's own table here: the first-stage paths, which hand this stage a table of ones, start at N = 32768)
  const bool w1 = e->win_ones && !exp_env("KSA_NO_W1");
  return with_fold(e, p, cfg_only, [&](auto cm) {
    constexpr int CM = decltype(cm)::value;
    return w1 ? launch_spec64_c<CM, true>(e, p, cfg_only) : launch_spec64_c<CM, false>(e, p, cfg_only);
  });
}

template <int FMT>
int launch_spec_n(ksa_engine* e, const SpecParams& p, bool cfg_only) {
  const int rm = p.nwin > 1 ? e->reuse_m : 0;   // RAW mode transforms a single window: nothing to reuse
  if (e->plan32) return e->sub_n == 8192 ? launch_spec32<8192, FMT>(e, p, cfg_only) : launch_spec32<16384, FMT>(e, p, cfg_only);
  return with_size(e->sub_n, [&](auto size) {
    constexpr int N = decltype(size)::value;
    if constexpr (N == 64 && FMT == ksa::FMT_C64) {
      if (e->k64_ok) {
        if (cfg_only) { if (launch_spec64(e, p, true)) return 1; }     // (then the general kernel's attributes too: uint8 input runs it)
        else if (!exp_env("KSA_NO_K64")) return launch_spec64(e, p, false);
      }
    }
    return launch_spec_rm<N, FMT>(e, p, cfg_only, rm);
  });
}

// fft_size 2^a * 3^b * 5^c (path 6): the mixed-radix kernel, one frame per workgroup at the plan's thread count.  It has no
// window split (p.parts): a one-frame batch runs on one workgroup.
template <int FMT>
int launch_mr(ksa_engine* e, const SpecParams& p, bool configure_only) {
  const bool psd = fold_psd(e);
  void (*kfn)(const SpecParams, const ksa::MrPlan);
  if constexpr (FMT == ksa::FMT_S8 || FMT == ksa::FMT_S16) kfn = psd ? ksa::mixed_radix_fixed_kernel<FMT, ksa::CUMU_PSD> : ksa::mixed_radix_fixed_kernel<FMT, 0>;
  else kfn = psd ? ksa::mixed_radix_psd_kernel<FMT> : ksa::mixed_radix_kernel<FMT>;
  const int lds_bytes = e->mr.n * (int)sizeof(float2);
  if (configure_only) {
    // (one kernel serves every N of the path: its attribute is set to the largest transform, not to this engine's)
    KernelFit fit;
    if (configure_kernel(kfn, e->threads, lds_bytes, &fit, 16384 * (int)sizeof(float2))) return 1;
    if (FMT == ksa::FMT_C64) {
      e->lds_bytes = lds_bytes;
      e->vgprs = fit.vgprs;
      e->blocks_per_cu = fit.blocks_per_cu;
    }
    return 0;
  }
  const int grid = std::max(1, std::min(p.nframes, e->num_cu * e->blocks_per_cu));
  hipLaunchKernelGGL(kfn, dim3(grid), dim3(e->threads), lds_bytes, e->stream, p, e->mr);
  HIP_OK(hipGetLastError());
  return 0;
}

// Configure pass of an engine: every kernel a later call of any sample format can launch.
int configure_kernels(ksa_engine* e, int num_windows) {
  SpecParams dummy{};
  dummy.nwin = num_windows;
  return for_each_fmt(Formats{}, [&](auto f) {
    constexpr int FMT = decltype(f)::value;
    return e->path == 6 ? launch_mr<FMT>(e, dummy, true) : launch_spec_n<FMT>(e, dummy, true);
  });
}

// The samples a spectrum-stage call is handed: `nframes` frames from `iq`, `stride` samples apart.  They are frames
// [batch_first, batch_first + nframes) of a batch of batch_frames (0: nframes; run_spectrum resolves it) whose launch plan,
// ring rows and ring window the call takes: slot by slot (a host batch) or chunk by chunk it writes what one call over the
// batch writes.
struct Frames {
  const void* iq;
  int fmt;
  long long stride;
  int nframes;
  int batch_first = 0, batch_frames = 0;
};

template <int FMT>
int launch_pfb_fmt(ksa_engine* e, const ksa::PfbParams& a, bool ring) {
  const long long per = a.n / ksa::PFB_COLS;
  if (ring) {
    const long long items = per * ((a.nframes + ksa::PFB_SLICE_FRAMES - 1) / ksa::PFB_SLICE_FRAMES);
    const dim3 grid((unsigned)((items + ksa::PFB_THREADS - 1) / ksa::PFB_THREADS));
    // (only the (format, P) pairs the rule below can select are instantiated: ksa::pfb_ring_pays)
    if constexpr (ksa::pfb_ring_pays(FMT, 4)) {
      if (a.ntaps == 4) hipLaunchKernelGGL((ksa::pfb_ring_kernel<FMT, 4>), grid, dim3(ksa::PFB_THREADS), 0, e->stream, a);
    }
    if (a.ntaps == 8) hipLaunchKernelGGL((ksa::pfb_ring_kernel<FMT, 8>), grid, dim3(ksa::PFB_THREADS), 0, e->stream, a);
    if (a.ntaps == 16) hipLaunchKernelGGL((ksa::pfb_ring_kernel<FMT, 16>), grid, dim3(ksa::PFB_THREADS), 0, e->stream, a);
  } else {
    const long long items = per * a.nframes;
    const long long blocks = (items + ksa::PFB_THREADS - 1) / ksa::PFB_THREADS;
    const dim3 grid((unsigned)std::max<long long>(1, std::min<long long>(blocks, (long long)e->num_cu * 32)));
    hipLaunchKernelGGL(ksa::pfb_fold_kernel<FMT>, grid, dim3(ksa::PFB_THREADS), 0, e->stream, a);
  }
  HIP_OK(hipGetLastError());
  return 0;
}

// KSA_CUMU_PFB_PSD: the block-aware kernels, a.f.nframes blocks of a.nsub sub-frames each.
template <int FMT>
int launch_pfbpsd_fmt(ksa_engine* e, const ksa::PfbPsdParams& a, bool ring) {
  const long long per = a.f.n / ksa::PFB_COLS;
  if (ring) {
    const long long slices = (a.nsub + ksa::PFB_SLICE_FRAMES - 1) / ksa::PFB_SLICE_FRAMES;
    const long long items = per * slices * a.f.nframes;
    const dim3 grid((unsigned)((items + ksa::PFB_THREADS - 1) / ksa::PFB_THREADS));
    // (only the (format, P) pairs the rule can select are instantiated: ksa::pfbpsd_ring_pays)
    bool launched = false;
    dispatch(a.f.ntaps, Ints<4, 8, 16>{}, [&](auto taps) {
      constexpr int P = decltype(taps)::value;
      if constexpr (ksa::pfbpsd_ring_pays(FMT, P)) {
        hipLaunchKernelGGL((ksa::pfbpsd_ring_kernel<FMT, P>), grid, dim3(ksa::PFB_THREADS), 0, e->stream, a);
        launched = true;
      }
      return 0;
    });
    if (!launched) return fail("no block ring kernel for format %d at %d taps", FMT, a.f.ntaps);
  } else {
    const long long items = per * a.nsub * a.f.nframes;
    const long long blocks = (items + ksa::PFB_THREADS - 1) / ksa::PFB_THREADS;
    const dim3 grid((unsigned)std::max<long long>(1, std::min<long long>(blocks, (long long)e->num_cu * 32)));
    hipLaunchKernelGGL(ksa::pfbpsd_fold_kernel<FMT>, grid, dim3(ksa::PFB_THREADS), 0, e->stream, a);
  }
  HIP_OK(hipGetLastError());
  return 0;
}

// One fold launch of a KSA_CUMU_PFB / KSA_CUMU_PFB_PSD engine: the caller's frames `f` (at most pfb_chunk) ->
// d_pfb_y[nframes][N], or d_pfb_y[nframes][K][N] on a KSA_CUMU_PFB_PSD engine.
int launch_pfb(ksa_engine* e, const Frames& f) {
  const ksa_config& c = e->cfg;
  ksa::PfbParams a{};
  a.iq = f.iq;
  a.frame_stride = f.stride;
  a.nframes = f.nframes;
  a.n = c.fft_size;
  a.ntaps = c.num_windows;
  a.starts = e->d_pfb_starts;
  a.taps = e->d_pfb_taps;
  a.u8_offset = c.u8_offset;
  a.u8_inv_scale = 1.0f / c.u8_scale;
  a.y = e->d_pfb_y;
  if (fold_pfb_psd(e)) {
    // The sliding happens inside a block, so the ring form serves every frame_stride (KSA_PFB_NO_RING: A/B switch of the
    // experiments build).
    const bool ring = e->pfb_ring_ok && ksa::pfbpsd_ring_pays(f.fmt, c.num_windows) && !exp_env("KSA_PFB_NO_RING");
    const ksa::PfbPsdParams b{a, e->pfb_sub};
    return with_fmt(f.fmt, [&](auto fmt) { return launch_pfbpsd_fmt<decltype(fmt)::value>(e, b, ring); });
  }
  // The ring kernel where it measured faster than the generic one at stride N (profiles/pfb_sweep.txt): it saves (P - 1)
  // re-reads of a sample per output point and pays with P - 1 warm-up loads per slice and fewer, longer threads; from 12 saved
  // bytes up it won (complex64 P >= 4, 2-byte samples P >= 8), below that the generic kernel's re-reads hit in cache and it lost.
  // (KSA_PFB_NO_RING: A/B switch of the experiments build.)
  const bool ring = e->pfb_ring_ok && f.stride == c.fft_size && ksa::pfb_ring_pays(f.fmt, c.num_windows) && !exp_env("KSA_PFB_NO_RING");
  return with_fmt(f.fmt, [&](auto fmt) { return launch_pfb_fmt<decltype(fmt)::value>(e, a, ring); });
}

int prof_begin(ksa_engine* e, hipEvent_t* a, hipEvent_t* b) {
  *a = *b = nullptr;
  if (!e->prof || e->prof_events.size() >= 8192) return 0;
  HIP_OK(hipEventCreate(a));
  HIP_OK(hipEventCreate(b));
  HIP_OK(hipEventRecord(*a, e->stream));
  return 0;
}
int prof_end(ksa_engine* e, hipEvent_t a, hipEvent_t b) {
  if (!a) return 0;
  HIP_OK(hipEventRecord(b, e->stream));
  e->prof_events.emplace_back(a, b);
  return 0;
}

// N = 16 * N1 (32768 .. 262144): first stage in registers, N1-point stage by the single-workgroup kernel on the
// 16 pseudo frames of every frame, interleave + dB + waterfall by dif16_finish_kernel (ksa_dif16.hpp).
// Chunks of dif_chunk frames are counted from frame 0 of the whole batch (this call holds its frames [batch_first,
// batch_first + nframes) of batch_frames): a host batch that arrives slot by slot gets the chunks, and so the second-stage
// plans, of one call over the whole batch.
int run_dif16(ksa_engine* e, const SpecParams& p, int fmt, int batch_first, int batch_frames) {
  const int n = e->cfg.fft_size, n1 = e->sub_n, nwin = p.nwin;
  for (int f0 = 0, cf = 0; f0 < p.nframes; f0 += cf) {
    const int g0 = batch_first + f0, chunk0 = g0 - g0 % e->dif_chunk;
    const int chunk_frames = std::min(e->dif_chunk, batch_frames - chunk0);
    cf = std::min(chunk0 + chunk_frames - g0, p.nframes - f0);
    ksa::DifParams a{};
    a.iq = p.iq;
    a.frame_stride = p.frame_stride;
    a.frame0 = f0;
    a.nwin = nwin;
    a.starts = p.starts;
    a.window = p.window;
    a.tw = e->d_dif_tw;
    a.n1 = n1;
    a.u8_offset = p.u8_offset;
    a.u8_inv_scale = p.u8_inv_scale;
    a.z = e->d_dif_z;
    const int R = e->dif_radix;
    if (with_fmt(fmt, [&](auto f) {
          constexpr int FMT = decltype(f)::value;
          return dispatch(R, Radices{}, [&](auto radix) {
            constexpr int RX = decltype(radix)::value;
            if constexpr (RX == 16)     // two adjacent n1 per thread
              hipLaunchKernelGGL(ksa::dif16_kernel<FMT>, dim3(n1 / 512, nwin, cf), dim3(256), 0, e->stream, a);
            else                        // one n1 per thread, 32 or 64 samples in registers
              hipLaunchKernelGGL((ksa::dif_wide_kernel<FMT, RX>), dim3(n1 / 256, nwin, cf), dim3(256), 0, e->stream, a);
            return 0;
          });
        })) return 1;
    SpecParams b{};
    b.iq = e->d_dif_z;
    b.frame_stride = (long long)nwin * n1;
    b.frame_len = nwin * n1;
    b.nframes = cf * R;
    b.nwin = nwin;
    b.starts = e->d_starts_b;      // w * N1 (a single window, RAW mode, starts at 0 too)
    b.window = e->d_ones;
    b.tw_mid = p.tw_mid;
    b.tw_last = p.tw_last;
    b.scale = p.scale;
    b.cumu = p.cumu;
    b.out_mode = ksa::OUT_LINEAR;
    b.out = e->d_dif_y;
    b.dbg = p.dbg;                 // (diagnostic builds: the second stage's records; null otherwise)
    e->plan_frames = chunk_frames * R;
    if (launch_spec_n<ksa::FMT_C64>(e, b, false)) return 1;
    ksa::DifFinishParams c{};
    c.y = e->d_dif_y;
    c.n = n;
    c.n1 = n1;
    c.radix = R;
    c.frame0 = f0;
    c.out_mode = p.out_mode;
    c.gain = p.gain;
    c.min_amp = p.min_amp;
    c.out = p.out;
    c.hm_w = p.hm_w;
    c.adj = p.adj;
    c.hm_rows = p.hm_rows;
    c.hm_ring = p.hm_ring;
    c.hm_index0 = p.hm_index0;
    c.hm_first = p.hm_first;
    dispatch(R, Radices{}, [&](auto radix) {
      hipLaunchKernelGGL(ksa::dif16_finish_kernel<decltype(radix)::value>, dim3(n1 / (1024 / R), cf), dim3(256), 0, e->stream, c);
      return 0;
    });
  }
  if (p.hm_w > 0 && n / p.hm_w > 1024)      // cells wider than the finish kernel's tile
    hipLaunchKernelGGL(ksa::rowmax_batch, dim3((p.hm_w + 255) / 256, p.nframes), dim3(256), 0, e->stream, p, n);
  HIP_OK(hipGetLastError());
  return 0;
}

// What every spectrum-stage call checks on the samples it is handed (the caller's, or a chunk of folded frames).
int check_frames(const ksa_engine* e, const Frames& f, const float* out, const float* hm_rows) {
  const ksa_config& c = e->cfg;
  if (f.fmt != KSA_FMT_C64 && f.fmt != KSA_FMT_U8 && f.fmt != KSA_FMT_S8 && f.fmt != KSA_FMT_S16) return fail("unknown sample format %d", f.fmt);
  if (f.nframes < 1 || f.nframes > c.max_frames) return fail("nframes %d outside 1..max_frames(%d)", f.nframes, c.max_frames);
  if (f.stride < 0) return fail("negative frame_stride");
  if (f.stride > (1ll << 27)) return fail("frame_stride %lld exceeds 2^27 samples", f.stride);
  // the output stage stores float4 runs; IQ loads are per-sample but frames should start on sample bounds
  if ((reinterpret_cast<uintptr_t>(out) & 15) || (hm_rows && (reinterpret_cast<uintptr_t>(hm_rows) & 15)))
    return fail("device output buffers must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(f.iq) & (sample_bytes(f.fmt) - 1)) return fail("IQ buffer is not sample aligned");
  return 0;
}

// Spectrum stage for a batch: the single-workgroup LDS FFT, behind a radix-16 / 32 / 64 first stage for N > 16384.
// `fold` (KSA_CUMU_PFB, KSA_CUMU_PFB_PSD): the fold launch that fills f.iq for these frames, enqueued inside the profiled
// interval; the frames are then folded ones of pfb_sub rectangular windows each (one on a KSA_CUMU_PFB engine).
int run_transform(ksa_engine* e, const Frames& f, int out_mode, float* out, bool with_hm, float* hm_rows, const Frames* fold) {
  const ksa_config& c = e->cfg;
  if (check_frames(e, f, out, hm_rows)) return 1;
  SpecParams p{};
  p.iq = f.iq;
  p.frame_stride = f.stride;
  p.frame_len = fold ? e->pfb_sub * c.fft_size : c.full_size;
  p.nframes = f.nframes;
  const bool raw = c.cumu_mode == KSA_CUMU_RAW;
  p.nwin = fold ? e->pfb_sub : raw ? 1 : c.num_windows;  // RAW keeps the last window only (K:135-136); a folded frame is one window (KSA_CUMU_PFB_PSD: K)
  p.starts = raw ? e->d_start_last : e->d_starts;
#if defined(KSA32_TAPS_X4) && !KSA32_TAPS_X4
  p.window = e->d_window;
#else
  p.window = (e->plan32 && e->path == 0) ? e->d_window32 : e->d_window;
#endif
  p.tw_mid = e->d_tw_mid;
  p.tw_last = e->d_tw_last;
  p.scale = (float)c.mag_scale;
  p.cumu = (raw || fold || c.cumu_mode == KSA_CUMU_AVG || c.cumu_mode == KSA_CUMU_PSD) ? ksa::CUMU_AVG : c.cumu_mode == KSA_CUMU_MAX ? ksa::CUMU_MAX : ksa::CUMU_MIN;
  p.out_mode = out_mode;
  p.gain = c.gain;
  p.min_amp = c.min_amp;
  p.u8_offset = c.u8_offset;
  p.u8_inv_scale = 1.0f / c.u8_scale;
  p.out = out;
  p.hm_w = with_hm ? c.hm_width : 0;
  p.adj = with_hm ? e->d_adj : nullptr;
  p.hm_rows = with_hm ? hm_rows : nullptr;
  p.hm_ring = with_hm ? e->d_hm : nullptr;
  p.hm_index0 = (e->hm_index + f.batch_first) % KSA_HM_ROWS;
  p.hm_first = std::max(0, f.batch_frames - KSA_HM_ROWS - f.batch_first);
  e->plan_frames = f.batch_frames;
#ifdef KSA_SKEW
  static unsigned long long* dbg = nullptr;   // diagnostic build: 4096 blocks x 16 waves x 12 segments, then 4096 workgroup records
  const size_t dbg_n = ksa::SKEW_SEG_WORDS, skew_n = (size_t)ksa::SKEW_WGS * 4;
  if (!dbg) hipMalloc(reinterpret_cast<void**>(&dbg), (dbg_n + skew_n) * 8);
  hipMemsetAsync(dbg, 0, (dbg_n + skew_n) * 8, e->stream);
  p.dbg = dbg;
#endif
  // profiled stage: clock stamps directly before and after it on the same stream (ksa_prof_clock), OUTSIDE the event pair
  ksa::u64x2* const clk = (e->prof && e->d_clk) ? reinterpret_cast<ksa::u64x2*>(e->d_clk) + (size_t)(e->clk_launches++ % ksa::CLK_SLOTS) * 2 * ksa::CLK_KEYS : nullptr;
  if (clk) hipLaunchKernelGGL(ksa::clock_stamp_kernel, dim3(ksa::CLK_WGS), dim3(64), 0, e->stream, clk, 0);
  hipEvent_t ea, eb;
  if (prof_begin(e, &ea, &eb)) return 1;
  if (fold && launch_pfb(e, *fold)) return 1;
  int rc;
  if (e->path == 2) rc = run_dif16(e, p, f.fmt, f.batch_first, f.batch_frames);
  else if (e->path == 6) rc = with_fmt(f.fmt, [&](auto fmt) { return launch_mr<decltype(fmt)::value>(e, p, false); });
  else rc = with_fmt(f.fmt, [&](auto fmt) { return launch_spec_n<decltype(fmt)::value>(e, p, false); });
  e->plan_frames = 0;
  if (rc) return rc;
#ifdef KSA_STAMPS
  if (const char* path = exp_env("KSA_STAMPS_FILE")) {
    hipStreamSynchronize(e->stream);
    std::vector<unsigned long long> h(dbg_n);
    hipMemcpy(h.data(), dbg, dbg_n * 8, hipMemcpyDeviceToHost);
    double sum[12] = {0};
    long long waves = 0;
    for (size_t w = 0; w < dbg_n / 12; ++w) {
      if (!h[w * 12 + 0] && !h[w * 12 + 7]) continue;
      ++waves;
      for (int i = 0; i < 12; ++i) sum[i] += (double)h[w * 12 + i];
    }
    if (FILE* fp = fopen(path, "a")) {
      fprintf(fp, "waves %lld nframes %d nwin %d :", waves, f.nframes, p.nwin);
      for (int i = 0; i < 12; ++i) fprintf(fp, " %.0f", waves ? sum[i] / waves : 0.0);
      fprintf(fp, "\n");
      fclose(fp);
    }
  }
#endif
  if (prof_end(e, ea, eb)) return 1;
  if (clk) hipLaunchKernelGGL(ksa::clock_stamp_kernel, dim3(ksa::CLK_WGS), dim3(64), 0, e->stream, clk, 1);
#ifdef KSA_SKEW
  // one line per workgroup of this call's (last) spectrum launch: "launch <k> <wg> <xcc> <start> <end> <units>", wall clock in
  // 100 MHz ticks; tools/ticket_skew.py turns them into first / median / last finish per XCD
  if (const char* path = getenv("KSA_SKEW_FILE")) {
    static int skew_launch = 0;
    hipStreamSynchronize(e->stream);
    std::vector<unsigned long long> h(skew_n);
    hipMemcpy(h.data(), dbg + dbg_n, skew_n * 8, hipMemcpyDeviceToHost);
    if (FILE* fp = fopen(path, "a")) {
      for (int w = 0; w < ksa::SKEW_WGS; ++w)
        if (h[w * 4 + 1])
          fprintf(fp, "launch %d %d %llu %llu %llu %llu\n", skew_launch, w, h[w * 4 + 3], h[w * 4 + 0], h[w * 4 + 1], h[w * 4 + 2]);
      fclose(fp);
    }
    ++skew_launch;
  }
#endif
  return 0;
}

// Spectrum stage of every entry point.  KSA_CUMU_PFB: the batch runs in chunks of pfb_chunk frames -- fold into the engine's
// scratch, then the transform on that scratch as complex64 frames of N samples at stride N -- and every chunk takes the whole
// batch's launch plan and ring rows (batch_first / batch_frames), exactly as the slots of a host batch do.  KSA_CUMU_PFB_PSD:
// the same in whole blocks, a folded frame being the K sub-frames of one block (K*N samples at stride K*N).
int run_spectrum(ksa_engine* e, Frames f, int out_mode, float* out, bool with_hm, float* hm_rows) {
  if (f.batch_frames < 1) f.batch_frames = f.nframes;
  if (!fold_time(e)) return run_transform(e, f, out_mode, out, with_hm, hm_rows, nullptr);
  const ksa_config& c = e->cfg;
  if (check_frames(e, f, out, hm_rows)) return 1;
  const size_t n = (size_t)c.fft_size;
  for (int f0 = 0; f0 < f.nframes; f0 += e->pfb_chunk) {
    const int nf = std::min(e->pfb_chunk, f.nframes - f0);
    const Frames fold{static_cast<const unsigned char*>(f.iq) + (size_t)f0 * (size_t)f.stride * sample_bytes(f.fmt), f.fmt, f.stride, nf};
    const Frames folded{e->d_pfb_y, KSA_FMT_C64, (long long)e->pfb_sub * c.fft_size, nf, f.batch_first + f0, f.batch_frames};
    if (run_transform(e, folded, out_mode, out + (size_t)f0 * n, with_hm, hm_rows ? hm_rows + (size_t)f0 * c.hm_width : nullptr, &fold)) return 1;
  }
  return 0;
}

int run_accumulate(ksa_engine* e, const float* db, int nframes, long long first_index, long long total) {
  const int n = e->cfg.fft_size;
  ksa::AccParams a{};
  a.db = db;
  a.n = n;
  a.nframes = nframes;
  a.first_index = first_index;
  a.total_frames = total;
  a.has_prev = e->has_avg;
  int chunks = std::min(e->max_chunks, std::max(1, nframes / 64));
  a.chunk = (nframes + chunks - 1) / chunks;
  chunks = (nframes + a.chunk - 1) / a.chunk;
  a.part = e->d_part;
  const int tb = 256, gx = (n + tb - 1) / tb;
  const int tb4 = 64, gx4 = (n / 4 + tb4 - 1) / tb4;     // 4 bins per thread
  hipLaunchKernelGGL(ksa::accumulate_partial_kernel, dim3(gx4, chunks), dim3(tb4), 0, e->stream, a);
  const int owns_last = first_index + nframes == total;
  hipLaunchKernelGGL(ksa::accumulate_reduce_kernel, dim3((n + 63) / 64), dim3(1024), 0, e->stream, e->d_part, chunks, n,
                     db + (long long)(nframes - 1) * n, owns_last, e->d_partial);
  HIP_OK(hipGetLastError());
  return 0;
}

int do_commit(ksa_engine* e, long long total, int local_frames) {
  const int n = e->cfg.fft_size;
  const int tb = 256, gx = (n + tb - 1) / tb;
  hipLaunchKernelGGL(ksa::commit_kernel, dim3(gx), dim3(tb), 0, e->stream, e->d_partial, e->d_state, n,
                     e->has_max, e->has_min, e->has_avg, total, e->b_max, e->b_min, e->b_avg);
  HIP_OK(hipGetLastError());
  e->has_max |= e->b_max;
  e->has_min |= e->b_min;
  e->has_avg |= e->b_avg;
  e->frames_seen += total;
  e->hm_index = (int)((e->hm_index + local_frames) % KSA_HM_ROWS);
  e->pending_frames = 0;
  return 0;
}

template <typename T>
int upload(T** dst, const T* src, size_t count) {
  HIP_OK(hipMalloc(reinterpret_cast<void**>(dst), std::max<size_t>(count, 1) * sizeof(T)));
  if (count) HIP_OK(hipMemcpy(*dst, src, count * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

int fill(ksa_engine* e, float* dst, long long n, float v) {
  if (n <= 0) return 0;
  const int tb = 256;
  const int gx = (int)std::min<long long>((n + tb - 1) / tb, 4096);
  hipLaunchKernelGGL(ksa::fill_kernel, dim3(gx), dim3(tb), 0, e->stream, dst, n, v);
  HIP_OK(hipGetLastError());
  return 0;
}

int scan_reset(ksa_engine* e) {
  const ksa_config& c = e->cfg;
  if (!c.scan_total_entries) return fail("engine was created without scan geometry");
  // K:603-608: Cur = Max = Avg = dB(minAmp4Clip), Min = dB(1.0); K:613-614 ring = minAmp4Clip (linear)
  float floor_db = (float)(10.0 * std::log10((double)c.min_amp) - (double)c.gain);
  if (std::isinf(floor_db)) floor_db = 0.f;      // infTo = 0 (K:604 -> K:110-111): minAmp4Clip 0 starts the curves at 0 dB
  const float one_db = (float)(10.0 * std::log10(1.0) - (double)c.gain);
  const long long t = c.scan_total_entries;
  if (fill(e, e->d_scan_state, t, floor_db)) return 1;
  if (fill(e, e->d_scan_state + t, t, floor_db)) return 1;
  if (fill(e, e->d_scan_state + 2 * t, t, one_db)) return 1;
  if (fill(e, e->d_scan_state + 3 * t, t, floor_db)) return 1;
  if (fill(e, e->d_scan_hm, (long long)KSA_HM_ROWS * c.scan_hm_width, c.min_amp)) return 1;
  e->scan_passes = 0;
  e->scan_hm_index = 0;
  e->scan_rows = e->scan_rows_passes = 0;      // an abandoned band-sharded batch must not block ksa_scan_allstitch for ever
  return 0;
}

// Grow-only device scratch of an engine (on its device, which the caller has made current).
template <typename T>
int ensure(T** ptr, size_t* cap, size_t count) {
  if (*ptr && *cap >= count) return 0;
  if (*ptr) hipFree(*ptr);
  *ptr = nullptr;
  *cap = 0;
  HIP_OK(hipMalloc(reinterpret_cast<void**>(ptr), std::max<size_t>(count, 1) * sizeof(T)));
  *cap = count;
  return 0;
}

// KSA_CUMU_PFB_PSD: K, the sub-frames of fft_size samples a block holds behind its last segment start (include/ksa.h); at
// least 1 once the starts have passed their check against full_size.
int pfb_subframes(const ksa_config* cfg) {
  const int n = cfg->fft_size;
  const int last = *std::max_element(cfg->window_starts, cfg->window_starts + cfg->num_windows);
  return (cfg->full_size - last - n) / n + 1;
}

// ---- ksa_create, step by step ------------------------------------------------------------------------------------------------
// 1. the checks that need no device
int validate_config(const ksa_config* cfg) {
  if (cfg->abi_version != KSA_ABI_VERSION) return fail("ABI version %d, library is %d", cfg->abi_version, KSA_ABI_VERSION);
  const int n = cfg->fft_size;
  const bool mixed = is_mixed_radix(n);
  if (!mixed && (!is_pow2(n) || n < 16 || n > (1 << 20)))
    return fail("fft_size %d must be a power of two in 16..1048576, or 2^a*3^b*5^c, a multiple of 4, in 16..16384", n);
  if (cfg->full_size < n) return fail("full_size %d < fft_size %d", cfg->full_size, n);
  // the spectrum kernels address a block in bytes with 32-bit offsets ((start + l) * SB, frame_len * SB): the bound is that of
  // the widest sample (complex64, 8 bytes) so that it holds whatever `fmt` a later call names
  if (cfg->full_size > KSA_MAX_FULL_SIZE)
    return fail("full_size %d exceeds %d samples (32-bit byte offsets of 8-byte samples)", cfg->full_size, KSA_MAX_FULL_SIZE);
  if (cfg->num_windows < 1 || !cfg->window_starts || !cfg->window) return fail("window table / starts missing");
  for (int i = 0; i < cfg->num_windows; ++i)
    if (cfg->window_starts[i] < 0 || (long long)cfg->window_starts[i] + n > (long long)cfg->full_size)
      return fail("window_starts[%d] = %d: the window [%d, %lld) lies outside the block of full_size %d", i, cfg->window_starts[i],
                  cfg->window_starts[i], (long long)cfg->window_starts[i] + n, cfg->full_size);
  if (cfg->cumu_mode < KSA_CUMU_RAW || cfg->cumu_mode > KSA_CUMU_PFB_PSD) return fail("unknown cumu_mode %d", cfg->cumu_mode);
  if (cfg->cumu_mode == KSA_CUMU_PFB && cfg->num_windows > KSA_PFB_MAX_TAPS)
    return fail("KSA_CUMU_PFB: num_windows %d outside 1..%d taps", cfg->num_windows, KSA_PFB_MAX_TAPS);
  if (cfg->cumu_mode == KSA_CUMU_PFB_PSD) {
    if (cfg->num_windows > KSA_PFB_MAX_TAPS)
      return fail("KSA_CUMU_PFB_PSD: num_windows %d outside 1..%d taps", cfg->num_windows, KSA_PFB_MAX_TAPS);
    // one block's folded sub-frames must fit a fold + transform chunk
    const long long bytes = (long long)pfb_subframes(cfg) * n * 8;
    if (bytes > (long long)KSA_PFB_CHUNK_BYTES)
      return fail("KSA_CUMU_PFB_PSD: %lld bytes of folded sub-frames per block (%d x fft_size %d x 8) exceed the chunk of %lld bytes",
                  bytes, pfb_subframes(cfg), n, (long long)KSA_PFB_CHUNK_BYTES);
  }
  if (mixed && (cfg->hm_width < 0 || (cfg->hm_width && n % cfg->hm_width)))
    return fail("hm_width %d must divide fft_size %d", cfg->hm_width, n);
  if (!mixed && (cfg->hm_width < 0 || (cfg->hm_width && (n % cfg->hm_width || !is_pow2(cfg->hm_width)))))
    return fail("hm_width %d must be a power of two dividing fft_size", cfg->hm_width);
  if (cfg->max_frames < 1) return fail("max_frames must be >= 1");
  if (!std::isfinite(cfg->u8_scale) || cfg->u8_scale == 0.f) return fail("u8_scale %g must be finite and non-zero", (double)cfg->u8_scale);
  // the stitch, row and levels kernels index the state [4][scan_total_entries] in int: 3 * total + element < 2^31
  if (cfg->scan_total_entries < 0 || cfg->scan_total_entries > KSA_MAX_SCAN_TOTAL_ENTRIES)
    return fail("scan_total_entries %d outside 0..%d", cfg->scan_total_entries, KSA_MAX_SCAN_TOTAL_ENTRIES);
  if (cfg->scan_total_entries) {
    if (cfg->scan_hop < 1 || cfg->scan_hop > n) return fail("scan_hop %d outside 1..fft_size", cfg->scan_hop);
    if (cfg->scan_hm_width < 1 || cfg->scan_total_entries % cfg->scan_hm_width)
      return fail("scan_hm_width %d must divide scan_total_entries %d", cfg->scan_hm_width, cfg->scan_total_entries);
  }
  return 0;
}

// What the transform stage plans from and runs on: the caller's windows or, on a KSA_CUMU_PFB engine, the inner shape -- one
// window at start 0 with all-ones taps over a folded frame of N samples (the caller's starts and taps [P][N] belong to the fold).
// KSA_CUMU_PFB_PSD: K windows at j*N with all-ones taps over a folded frame of K*N samples.
struct WindowShape {
  int num_windows;
  const int32_t* starts;
  const float* taps;
};

// 2. path and plan: which kernels serve the engine (no HIP call)
void choose_plan(ksa_engine* e, const ksa_config* cfg, const WindowShape& w) {
  const int n = cfg->fft_size;
  e->win_ones = std::all_of(w.taps, w.taps + n, [](float t) { return t == 1.0f; });
  if (fold_time(e)) {
    const int p = cfg->num_windows;
    e->pfb_ring_ok = p == 4 || p == 8 || p == 16;
    for (int k = 0; k < p; ++k) e->pfb_ring_ok &= (long long)cfg->window_starts[k] == (long long)k * n;
    e->pfb_sub = fold_pfb_psd(e) ? w.num_windows : 1;
    // whole frames (KSA_CUMU_PFB_PSD: whole blocks of K sub-frames), a multiple of 4 (even for the pair kernel, 16-byte aligned
    // waterfall row offsets), at least 4
    const long long chunk = std::max<long long>(4, (long long)KSA_PFB_CHUNK_BYTES / ((long long)e->pfb_sub * n * 8) / 4 * 4);
    e->pfb_chunk = (int)std::min<long long>(chunk, ((long long)cfg->max_frames + 3) / 4 * 4);
  }
  if (is_mixed_radix(n)) {
    e->path = 6;
    e->sub_n = n;
    return;
  }
  e->path = n <= 16384 ? 0 : 2;
  e->dif_radix = n <= 262144 ? 16 : n == 524288 ? 32 : 64;
  const int sn = e->path == 0 ? n : n / e->dif_radix;     // the single-workgroup transform
  e->sub_n = sn;
  e->plan32 = (sn == 8192 || sn == 16384) && !exp_env("KSA_PLAN16");   // KSA_PLAN16 (experiments build): back to the 16-point plan
  // Two frames per workgroup in packed fp32 (ksa_kernels_pair.hpp).  Measured against the one-frame kernel on MI355X
  // (tools/pair_sweep.sh, hops 0.5 / 0.25 / 0.1): N = 1024 +14..+30 %, N = 2048 -3..-5 %, N = 4096 0..-5 % -- on by
  // default for 1024 only.  KSA_PAIR_ALL enables it for 1024 .. 4096, KSA_NO_PAIR disables it (A/B switches).
  e->pair_ok = e->path == 0 && !exp_env("KSA_NO_PAIR") && (sn == 1024 || (exp_env("KSA_PAIR_ALL") && sn >= 1024 && sn <= 4096));
  e->k64_ok = sn == 64 && e->path == 0;     // the 8 x 8 plan of N = 64 (ksa_kernels64.hpp)
  // constant hop of 1/2 or 1/4 of the transform: raw samples are carried over in registers
  if (e->path == 0 && w.num_windows > 1 && n >= 1024) {
    const int hop = w.starts[1] - w.starts[0];
    bool same = true;
    for (int i = 2; i < w.num_windows; ++i) same &= w.starts[i] - w.starts[i - 1] == hop;
    if (same && (hop == n / 2 || hop == n / 4)) e->reuse_m = hop / (n / 16);
  }
  if (exp_env("KSA_NO_REUSE")) e->reuse_m = 0;   // A/B switch of the experiments build
}

template <typename T>
int upload(T** dst, const std::vector<T>& src) { return upload(dst, src.data(), src.size()); }

// 3. the tables of the plan (ksa_tables.hpp), built and uploaded
int upload_tables(ksa_engine* e, const ksa_config* cfg, const WindowShape& w) {
  namespace tab = ksa::tables;
  const int n = cfg->fft_size, sn = e->sub_n;
  if (fold_time(e)) {
    if (upload(&e->d_pfb_starts, cfg->window_starts, (size_t)cfg->num_windows)) return 1;
    if (upload(&e->d_pfb_taps, cfg->window, (size_t)cfg->num_windows * n)) return 1;
  }
  if (upload(&e->d_starts, w.starts, (size_t)w.num_windows)) return 1;
  if (upload(&e->d_start_last, w.starts + w.num_windows - 1, 1)) return 1;
  if (upload(&e->d_window, w.taps, (size_t)n)) return 1;
  if (e->path == 6) {       // the plan's twiddles live in d_tw_mid
    std::vector<float2> tw;
    const std::string err = tab::plan_mr(n, &e->mr, &e->threads, &tw);
    if (!err.empty()) return fail("%s", err.c_str());
    if (upload(&e->d_tw_mid, tw)) return 1;
    e->mr.tw = e->d_tw_mid;
    return 0;
  }
  tab::Twiddles tw;
  if (e->plan32) {
    tw = tab::twiddles32(sn);
    if (upload(&e->d_window32, tab::taps32(sn, e->path == 0 ? w.taps : nullptr))) return 1;
  } else {
    bool fused_mid = false, fused_last = false;     // the table layouts are the kernel's own choice
    if (with_size(sn, [&](auto size) {
          using Tune = ksa::Tune<decltype(size)::value>;
          fused_mid = Tune::FUSED;
          fused_last = Tune::FUSED_LAST;
          return 0;
        })) return 1;
    tw = tab::twiddles16(sn, fused_mid, fused_last);
  }
  if (e->k64_ok) tw.mid = tab::twiddles64();     // the 4 x 16 plan of N = 64 has no middle pass, the slot is free
  if (upload(&e->d_tw_mid, tw.mid)) return 1;
  if (upload(&e->d_tw_last, tw.last)) return 1;
  if (e->path == 2) {
    if (upload(&e->d_dif_tw, tab::first_stage_twiddles(n, e->dif_radix))) return 1;
    if (upload(&e->d_ones, std::vector<float>((size_t)sn, 1.0f))) return 1;     // the window was applied in the first stage
    std::vector<int> sb((size_t)w.num_windows);
    for (int i = 0; i < w.num_windows; ++i) sb[i] = i * sn;
    if (upload(&e->d_starts_b, sb)) return 1;
  }
  return 0;
}

// 5. scratch (after the configure pass: the window split is sized by blocks_per_cu)
int alloc_scratch(ksa_engine* e, int num_windows) {
  const ksa_config& c = e->cfg;
  const int n = c.fft_size;
  const size_t nn = (size_t)n;
  hipError_t he;
  const size_t folded = (size_t)e->pfb_chunk * e->pfb_sub * n * sizeof(float2);
  if (fold_time(e) && (he = hipMalloc(reinterpret_cast<void**>(&e->d_pfb_y), folded)) != hipSuccess)
    return fail("hipMalloc(%zu) for the folded frames: %s", folded, hipGetErrorString(he));
  if (e->path == 2) {
    const int n1 = e->sub_n, nw = num_windows;
    // scratch: Z = 8 N bytes per window.  Chunks of <= KSA_FS_SCRATCH_MB (default below) of Z
    const size_t per_frame = (size_t)nw * n * sizeof(float2);
    // 32-bit offsets inside the kernels: a pseudo frame is nwin*N1 complex points addressed in bytes
    if ((long long)nw * n1 >= (1ll << 28)) return fail("num_windows %d x fft_size/16 %d exceeds 2^28 points per frame", nw, n1);
    size_t budget = (size_t)KSA_DIF_SCRATCH_MB_DEFAULT << 20;
    if (const char* mb = exp_env("KSA_FS_SCRATCH_MB")) {       // A/B switch of the experiments build; nonsense keeps the default
      const long v = atol(mb);
      if (v >= 1 && v <= (256l << 10)) budget = (size_t)v << 20;
    }
    e->dif_chunk = (int)std::min<size_t>(std::max<size_t>(1, budget / per_frame), (size_t)c.max_frames);
    e->dif_chunk = std::min(e->dif_chunk, 4095);               // gridDim.z of dif16_kernel, 16*chunk pseudo frames
    if ((he = hipMalloc(reinterpret_cast<void**>(&e->d_dif_z), per_frame * e->dif_chunk)) != hipSuccess)
      return fail("hipMalloc(%zu) for the first-stage scratch: %s", per_frame * e->dif_chunk, hipGetErrorString(he));
    if ((he = hipMalloc(reinterpret_cast<void**>(&e->d_dif_y), (size_t)e->dif_chunk * n * 4)) != hipSuccess)
      return fail("hipMalloc for the second-stage output: %s", hipGetErrorString(he));
  }
  e->max_chunks = (int)std::max<size_t>(1, std::min<size_t>(128, (64u << 20) / (3 * nn * 4)));
#define ALLOC(ptr, bytes)                                                        \
  if ((he = hipMalloc(reinterpret_cast<void**>(&(ptr)), (bytes))) != hipSuccess) \
    return fail("hipMalloc(%zu) for %s: %s", (size_t)(bytes), #ptr, hipGetErrorString(he));
  ALLOC(e->d_iq_stage, (size_t)c.full_size * 8);
  ALLOC(e->d_frames, (size_t)c.max_frames * nn * 4);
  ALLOC(e->d_part, (size_t)e->max_chunks * 3 * nn * 4);
  ALLOC(e->d_xchg, (4 * nn + (size_t)KSA_HM_ROWS * c.hm_width) * 4);
  e->d_partial = e->d_xchg;
  if (c.hm_width) e->d_hm = e->d_xchg + 4 * nn;
  ALLOC(e->d_state, 4 * nn * 4);
  if (e->path != 6) ALLOC(e->d_parts, (size_t)e->num_cu * e->blocks_per_cu * (size_t)e->sub_n * 4);   // (path 6 has no window split)
  ALLOC(e->d_tickets, sizeof(unsigned));
  if (c.scan_total_entries) {
    ALLOC(e->d_scan_state, (size_t)4 * c.scan_total_entries * 4);
    ALLOC(e->d_scan_hm, (size_t)KSA_HM_ROWS * c.scan_hm_width * 4);
  }
#undef ALLOC
  return 0;
}

}  // namespace

extern "C" {

int ksa_abi_version(void) { return KSA_ABI_VERSION; }
const char* ksa_last_error(void) { return g_err.c_str(); }

int ksa_create(const ksa_config* cfg, ksa_engine** out) {
  if (!cfg || !out) return fail("null argument");
  *out = nullptr;
  if (validate_config(cfg)) return 1;
  int ndev = 0;
  HIP_OK(hipGetDeviceCount(&ndev));
  if (cfg->device < 0 || cfg->device >= ndev) return fail("device %d not present (%d visible)", cfg->device, ndev);
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(cfg->device));
  hipDeviceProp_t prop;
  HIP_OK(hipGetDeviceProperties(&prop, cfg->device));

  ksa_engine* e = new ksa_engine();
  e->cfg = *cfg;
  e->cfg.window_starts = nullptr;
  e->cfg.window = nullptr;
  e->num_cu = prop.multiProcessorCount;
  auto bail = [&](int r) { ksa_destroy(e); return r; };

  const bool pfb = fold_time(e);
  const std::vector<float> pfb_ones(pfb ? (size_t)cfg->fft_size : 0, 1.0f);
  std::vector<int32_t> pfb_inner(fold_pfb_psd(e) ? (size_t)pfb_subframes(cfg) : 1);      // j*N (one window at 0 on a KSA_CUMU_PFB engine)
  for (size_t j = 0; j < pfb_inner.size(); ++j) pfb_inner[j] = (int32_t)j * cfg->fft_size;
  const WindowShape w = pfb ? WindowShape{(int)pfb_inner.size(), pfb_inner.data(), pfb_ones.data()}
                            : WindowShape{cfg->num_windows, cfg->window_starts, cfg->window};
  choose_plan(e, cfg, w);
  if (upload_tables(e, cfg, w)) return bail(1);
  if (configure_kernels(e, w.num_windows)) return bail(1);
  if (alloc_scratch(e, w.num_windows)) return bail(1);
  if (ksa_reset_state(e)) return bail(1);
  if (cfg->scan_total_entries && scan_reset(e)) return bail(1);
  if (hipStreamSynchronize(e->stream) != hipSuccess) return bail(fail("initial sync failed"));
  *out = e;
  return 0;
}

void ksa_destroy(ksa_engine* e) {
  if (!e) return;
  DeviceGuard dev_guard;
  hipSetDevice(e->cfg.device);
  hipDeviceSynchronize();
  for (auto& pr : e->prof_events) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
  for (hipEvent_t ev : {e->ev_ready, e->ev_copied, e->ev_stream, e->ev_copy_start, e->ev_slot_copied[0], e->ev_slot_copied[1],
                        e->ev_slot_read[0], e->ev_slot_read[1]})
    if (ev) hipEventDestroy(ev);
  if (e->copy_stream) hipStreamDestroy(e->copy_stream);
  void* ptrs[] = {e->d_slot[0], e->d_slot[1], e->d_host_rows, e->d_clk, e->d_gather, e->d_scan_stage, e->d_scan_rows, e->d_scan_halo, e->d_scan_send,
                  e->d_starts, e->d_start_last, e->d_window, e->d_window32, e->d_tw_mid, e->d_tw_last, e->d_adj, e->d_scan_adj,
                  e->d_iq_stage, e->d_frames, e->d_part, e->d_xchg, e->d_state, e->d_scan_state, e->d_scan_hm,
                  e->d_levels, e->d_parts, e->d_tickets, e->d_highs, e->d_scan_avg_rows, e->d_dif_tw, e->d_dif_z, e->d_dif_y, e->d_ones, e->d_starts_b,
                  e->d_pfb_starts, e->d_pfb_taps, e->d_pfb_y};
  for (void* p : ptrs) if (p) hipFree(p);
  delete e;
}

int ksa_set_stream(ksa_engine* e, void* hip_stream) {
  if (!e) return fail("null engine");
  hipStream_t ns = reinterpret_cast<hipStream_t>(hip_stream);
  if (ns == e->stream) return 0;
  // engine-owned buffers (state, scratch, rings) may still be in use on the old stream: order the new one behind it
  // (an event is recorded on the OLD stream, so a stream handed in here must stay alive until the next ksa_set_stream /
  //  ksa_destroy of this engine)
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(e->cfg.device));
  if (!e->ev_stream) HIP_OK(hipEventCreateWithFlags(&e->ev_stream, hipEventDisableTiming));
  HIP_OK(hipEventRecord(e->ev_stream, e->stream));
  HIP_OK(hipStreamWaitEvent(ns, e->ev_stream, 0));
  e->stream = ns;
  return 0;
}

int ksa_synchronize(ksa_engine* e) {
  if (!e) return fail("null engine");
  // (the default engine stream is the NULL stream, which means "the null stream of the CURRENT device": select the engine's)
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(e->cfg.device));
  HIP_OK(hipStreamSynchronize(e->stream));
  return 0;
}

int ksa_curscan_dev(ksa_engine* e, const void* iq_dev, int32_t fmt, int64_t frame_stride, int32_t nframes,
                    int32_t out_mode, float* out_dev) {
  if (!e || !iq_dev || !out_dev) return fail("null argument");
  if (out_mode < KSA_OUT_LINEAR || out_mode > KSA_OUT_DB_CLIP) return fail("unknown out_mode %d", out_mode);
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(e->cfg.device));
  return run_spectrum(e, {iq_dev, fmt, frame_stride, nframes}, out_mode, out_dev, false, nullptr);
}

static int curscan_host(ksa_engine* e, const void* iq_host, int fmt, float* mag_host) {
  if (!e || !iq_host || !mag_host) return fail("null argument");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(e->cfg.device));
  HIP_OK(hipMemcpyAsync(e->d_iq_stage, iq_host, (size_t)e->cfg.full_size * sample_bytes(fmt), hipMemcpyHostToDevice, e->stream));
  if (run_spectrum(e, {e->d_iq_stage, fmt, 0, 1}, KSA_OUT_LINEAR, e->d_frames, false, nullptr)) return 1;
  HIP_OK(hipMemcpyAsync(mag_host, e->d_frames, (size_t)e->cfg.fft_size * 4, hipMemcpyDeviceToHost, e->stream));
  HIP_OK(hipStreamSynchronize(e->stream));
  return 0;
}

int ksa_curscan_c64(ksa_engine* e, const float* iq_host, float* mag_host) { return curscan_host(e, iq_host, KSA_FMT_C64, mag_host); }
int ksa_curscan_u8(ksa_engine* e, const uint8_t* iq_host, float* mag_host) { return curscan_host(e, iq_host, KSA_FMT_U8, mag_host); }

int ksa_frames_dev(ksa_engine* e, const void* iq_dev, int32_t fmt, int64_t frame_stride, int32_t nframes,
                   int64_t first_index, int64_t total_frames, float* cur_db_dev, float* hm_rows_dev, int32_t commit) {
  if (!e || !iq_dev) return fail("null argument");
  if (first_index < 0 || first_index + nframes > total_frames) return fail("batch [%lld,+%d) outside run of %lld frames", (long long)first_index, nframes, (long long)total_frames);
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(e->cfg.device));
  float* db = cur_db_dev ? cur_db_dev : e->d_frames;
  if (run_spectrum(e, {iq_dev, fmt, frame_stride, nframes}, KSA_OUT_DB, db, e->cfg.hm_width > 0, hm_rows_dev)) return 1;
  if (run_accumulate(e, db, nframes, first_index, total_frames)) return 1;
  e->pending_frames = nframes;
  if (commit) return do_commit(e, total_frames, nframes);
  return 0;
}

static int frame_host(ksa_engine* e, const void* iq_host, int fmt) {
  if (!e || !iq_host) return fail("null argument");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(e->cfg.device));
  HIP_OK(hipMemcpyAsync(e->d_iq_stage, iq_host, (size_t)e->cfg.full_size * sample_bytes(fmt), hipMemcpyHostToDevice, e->stream));
  if (ksa_frames_dev(e, e->d_iq_stage, fmt, 0, 1, 0, 1, nullptr, nullptr, 1)) return 1;
  HIP_OK(hipStreamSynchronize(e->stream));
  return 0;
}

int ksa_frame_c64(ksa_engine* e, const float* iq_host) { return frame_host(e, iq_host, KSA_FMT_C64); }
int ksa_frame_u8(ksa_engine* e, const uint8_t* iq_host) { return frame_host(e, iq_host, KSA_FMT_U8); }

// A batch from host memory.  Its blocks cross PCIe slot by slot (include/ksa.h: KSA_FRAME_SLOT_BYTES) on the engine's copy
// stream into two device slots, while the engine's stream transforms the slot copied before; events order both ways (a slot's
// transform waits for its copy, the next copy into a slot waits for the transform that read it).  Every slot runs with the whole
// batch's launch plan and ring rows and writes its dB rows into d_frames at the batch position; ONE accumulate over the whole
// batch follows the last slot.  That is ksa_frames_dev on a device copy of the batch, bit for bit.
static int frames_host(ksa_engine* e, const void* iq_host, int fmt, int nframes, long long first_index, long long total,
                       float* cur_db_host, float* hm_rows_host, int commit) {
  if (!e || !iq_host) return fail("null argument");
  const ksa_config& c = e->cfg;
  if (nframes < 1 || nframes > c.max_frames) return fail("nframes %d outside 1..max_frames(%d)", nframes, c.max_frames);
  if (first_index < 0 || first_index + nframes > total) return fail("batch [%lld,+%d) outside run of %lld frames", first_index, nframes, total);
  if (hm_rows_host && !c.hm_width) return fail("hm_rows_host given, but the engine has no waterfall (hm_width 0)");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(c.device));
  const size_t n = (size_t)c.fft_size, frame_bytes = (size_t)c.full_size * sample_bytes(fmt);
  // whole frames, a multiple of 4 (even for the pair kernel, 16-byte aligned row offsets however narrow the waterfall), >= 4
  const int slot_frames = (int)std::max<size_t>(4, (size_t)KSA_FRAME_SLOT_BYTES / frame_bytes / 4 * 4);
  const size_t slot_bytes = (size_t)std::min(nframes, slot_frames) * frame_bytes;
  // scratch, stream and events before the first enqueue: a refusal up to here leaves the engine as it was
  for (int s = 0; s < 2; ++s)
    if (ensure(reinterpret_cast<unsigned char**>(&e->d_slot[s]), &e->slot_cap[s], slot_bytes)) return 1;
  if (hm_rows_host && ensure(&e->d_host_rows, &e->host_rows_cap, (size_t)nframes * c.hm_width)) return 1;
  if (!e->copy_stream) HIP_OK(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
  for (hipEvent_t* ev : {&e->ev_copy_start, &e->ev_slot_copied[0], &e->ev_slot_copied[1], &e->ev_slot_read[0], &e->ev_slot_read[1]})
    if (!*ev) HIP_OK(hipEventCreateWithFlags(ev, hipEventDisableTiming));
  // the first copy queues behind whatever the engine's stream holds (ksa_set_stream contract)
  HIP_OK(hipEventRecord(e->ev_copy_start, e->stream));
  HIP_OK(hipStreamWaitEvent(e->copy_stream, e->ev_copy_start, 0));
  float* const rows_dev = hm_rows_host ? e->d_host_rows : nullptr;
  for (int f0 = 0, k = 0; f0 < nframes; f0 += slot_frames, ++k) {
    const int nf = std::min(slot_frames, nframes - f0), s = k & 1;
    if (k >= 2) HIP_OK(hipStreamWaitEvent(e->copy_stream, e->ev_slot_read[s], 0));
    HIP_OK(hipMemcpyAsync(e->d_slot[s], static_cast<const unsigned char*>(iq_host) + (size_t)f0 * frame_bytes, (size_t)nf * frame_bytes,
                          hipMemcpyHostToDevice, e->copy_stream));
    HIP_OK(hipEventRecord(e->ev_slot_copied[s], e->copy_stream));
    HIP_OK(hipStreamWaitEvent(e->stream, e->ev_slot_copied[s], 0));
    if (run_spectrum(e, {e->d_slot[s], fmt, c.full_size, nf, f0, nframes}, KSA_OUT_DB, e->d_frames + (size_t)f0 * n, c.hm_width > 0,
                     rows_dev ? rows_dev + (size_t)f0 * c.hm_width : nullptr)) return 1;
    HIP_OK(hipEventRecord(e->ev_slot_read[s], e->stream));
  }
  if (run_accumulate(e, e->d_frames, nframes, first_index, total)) return 1;
  e->pending_frames = nframes;
  if (commit && do_commit(e, total, nframes)) return 1;
  if (cur_db_host) HIP_OK(hipMemcpyAsync(cur_db_host, e->d_frames, (size_t)nframes * n * 4, hipMemcpyDeviceToHost, e->stream));
  if (rows_dev) HIP_OK(hipMemcpyAsync(hm_rows_host, rows_dev, (size_t)nframes * c.hm_width * 4, hipMemcpyDeviceToHost, e->stream));
  HIP_OK(hipStreamSynchronize(e->stream));
  return 0;
}

int ksa_frames_c64(ksa_engine* e, const float* iq_host, int32_t nframes, int64_t first_index, int64_t total_frames,
                   float* cur_db_host, float* hm_rows_host, int32_t commit) {
  return frames_host(e, iq_host, KSA_FMT_C64, nframes, first_index, total_frames, cur_db_host, hm_rows_host, commit);
}
int ksa_frames_u8(ksa_engine* e, const uint8_t* iq_host, int32_t nframes, int64_t first_index, int64_t total_frames,
                  float* cur_db_host, float* hm_rows_host, int32_t commit) {
  return frames_host(e, iq_host, KSA_FMT_U8, nframes, first_index, total_frames, cur_db_host, hm_rows_host, commit);
}

int ksa_frame_spectrum(ksa_engine* e, const float* mag_host) {
  if (!e || !mag_host) return fail("null argument");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(e->cfg.device));
  const int n = e->cfg.fft_size;
  float* lin = reinterpret_cast<float*>(e->d_iq_stage);  // full_size*8 bytes >= N*4
  HIP_OK(hipMemcpyAsync(lin, mag_host, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
  ksa::DbRowParams p{};
  p.lin = lin;
  p.out = e->d_frames;
  p.n = n;
  p.nframes = 1;
  p.gain = e->cfg.gain;
  p.hm_w = e->cfg.hm_width;
  p.adj = e->d_adj;
  p.hm_rows = nullptr;
  p.hm_ring = e->d_hm;
  p.hm_index0 = e->hm_index;
  p.hm_first = 0;
  hipLaunchKernelGGL(ksa::db_rows_kernel, dim3(std::max(1, std::min(64, n / 256)), 1), dim3(256), 0, e->stream, p);
  HIP_OK(hipGetLastError());
  if (run_accumulate(e, e->d_frames, 1, 0, 1)) return 1;
  if (do_commit(e, 1, 1)) return 1;
  HIP_OK(hipStreamSynchronize(e->stream));
  return 0;
}

int ksa_partial_dev(ksa_engine* e, float** partial_dev) {
  if (!e || !partial_dev) return fail("null argument");
  *partial_dev = e->d_partial;
  return 0;
}

int ksa_exchange_dev(ksa_engine* e, float** xchg_dev, int64_t* nfloats) {
  if (!e || !xchg_dev || !nfloats) return fail("null argument");
  *xchg_dev = e->d_xchg;
  *nfloats = 4ll * e->cfg.fft_size + (long long)KSA_HM_ROWS * e->cfg.hm_width;
  return 0;
}

int ksa_merge_gathered_dev(ksa_engine* e, const float* gathered_dev, int32_t world, int32_t frames_per_rank,
                           int32_t hm_index0) {
  if (!e || !gathered_dev) return fail("null argument");
  if (world < 1) return fail("world %d < 1", world);
  if (frames_per_rank < 1) return fail("frames_per_rank %d < 1", frames_per_rank);
  if (e->pending_frames != frames_per_rank)
    return fail("ksa_merge_gathered_dev: %d frames pending, frames_per_rank says %d", e->pending_frames, frames_per_rank);
  if (hm_index0 < 0 || hm_index0 >= KSA_HM_ROWS) return fail("hm_index0 %d outside 0..127", hm_index0);
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(e->cfg.device));
  const int n = e->cfg.fft_size, w = e->cfg.hm_width;
  const long long stride = 4ll * n + (long long)KSA_HM_ROWS * w;
  const long long total = (long long)world * frames_per_rank;
  const long long cells = std::max<long long>(n, (long long)KSA_HM_ROWS * w);
  hipLaunchKernelGGL(ksa::merge_gathered_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, e->stream,
                     gathered_dev, world, stride, n, e->d_partial, e->d_hm, w, hm_index0, frames_per_rank, total);
  HIP_OK(hipGetLastError());
  if (do_commit(e, total, 0)) return 1;
  e->hm_index = (int)((hm_index0 + total) % KSA_HM_ROWS);
  return 0;
}

int ksa_commit(ksa_engine* e, int64_t total_frames) {
  if (!e) return fail("null engine");
  if (e->pending_frames <= 0) return fail("ksa_commit without a pending ksa_frames_dev(commit=0)");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(e->cfg.device));
  return do_commit(e, total_frames, e->pending_frames);
}

int ksa_set_flags(ksa_engine* e, int32_t b_max, int32_t b_min, int32_t b_avg) {
  if (!e) return fail("null engine");
  e->b_max = b_max != 0;
  e->b_min = b_min != 0;
  e->b_avg = b_avg != 0;
  return 0;
}

int ksa_set_adj(ksa_engine* e, int32_t scan, const float* adj_host, int32_t n) {
  if (!e) return fail("null engine");
  if (scan && !e->cfg.scan_total_entries) return fail("engine was created without scan geometry");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(e->cfg.device));
  HIP_OK(hipStreamSynchronize(e->stream));
  float** slot = scan ? &e->d_scan_adj : &e->d_adj;
  if (*slot) hipFree(*slot);
  *slot = nullptr;
  if (!adj_host) return 0;
  const int want = scan ? e->cfg.scan_total_entries : e->cfg.fft_size;
  if (n != want) return fail("adj length %d, the %s baseline needs %d", n, scan ? "scan" : "zeroSpan", want);
  return upload(slot, adj_host, (size_t)n);
}

int ksa_reset_state(ksa_engine* e) {
  if (!e) return fail("null engine");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(e->cfg.device));
  HIP_OK(hipMemsetAsync(e->d_state, 0, (size_t)4 * e->cfg.fft_size * 4, e->stream));
  if (e->d_hm) HIP_OK(hipMemsetAsync(e->d_hm, 0, (size_t)KSA_HM_ROWS * e->cfg.hm_width * 4, e->stream));  // np.zeros K:456
  e->frames_seen = 0;
  e->has_max = e->has_min = e->has_avg = 0;
  e->hm_index = 0;
  e->pending_frames = 0;
  return 0;
}

int ksa_read_state(ksa_engine* e, float* cur, float* max, float* min, float* avg, float* hm, int32_t* hm_index,
                   int64_t* frames_seen) {
  if (!e) return fail("null engine");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(e->cfg.device));
  if (hm && !e->d_hm) return fail("engine has no waterfall (hm_width 0)");      // (validated before the first copy is enqueued)
  const size_t nb = (size_t)e->cfg.fft_size * 4;
  float* dst[4] = {cur, max, min, avg};
  for (int i = 0; i < 4; ++i)
    if (dst[i]) HIP_OK(hipMemcpyAsync(dst[i], e->d_state + (size_t)i * e->cfg.fft_size, nb, hipMemcpyDeviceToHost, e->stream));
  if (hm) {
    HIP_OK(hipMemcpyAsync(hm, e->d_hm, (size_t)KSA_HM_ROWS * e->cfg.hm_width * 4, hipMemcpyDeviceToHost, e->stream));
  }
  HIP_OK(hipStreamSynchronize(e->stream));
  if (hm_index) *hm_index = e->hm_index;
  if (frames_seen) *frames_seen = e->frames_seen;
  return 0;
}

int ksa_state_dev(ksa_engine* e, float** state_dev, float** hm_ring_dev) {
  if (!e) return fail("null engine");
  if (state_dev) *state_dev = e->d_state;
  if (hm_ring_dev) *hm_ring_dev = e->d_hm;
  return 0;
}

int ksa_set_hm_index(ksa_engine* e, int32_t hm_index) {
  if (!e) return fail("null engine");
  if (hm_index < 0 || hm_index >= KSA_HM_ROWS) return fail("hm_index %d outside the ring", hm_index);
  e->hm_index = hm_index;
  return 0;
}

// Stitch + Max/Min/Avg over the elements [elem_lo, elem_hi) from the bands [step_lo, step_hi) (+ nhalo halo bands in
// front of them).  ranged == false: the whole range on one engine, the waterfall rows go straight into the ring;
// ranged == true: partial rows into d_scan_rows for ksa_scan_merge_rows_dev.
static int scan_stitch(ksa_engine* e, const float* step_db_dev, int nsteps, int npasses, bool ranged = false,
                       const float* halo_db_dev = nullptr, int nhalo = 0, int step_lo = 0, int step_hi = -1,
                       int elem_lo = 0, int elem_hi = -1, int own_band_major = 0) {
  if (!e || !step_db_dev) return fail("null argument");
  const ksa_config& c = e->cfg;
  if (!c.scan_total_entries) return fail("engine was created without scan geometry");
  if (nsteps < 1 || npasses < 1) return fail("nsteps and npasses must be >= 1");
  if (step_hi < 0) step_hi = nsteps;
  if (elem_hi < 0) elem_hi = c.scan_total_entries;
  HIP_OK(hipSetDevice(c.device));          // (the exported caller holds the DeviceGuard)
  ksa::StitchParams s{};
  s.step_db = step_db_dev;
  s.halo_db = halo_db_dev;
  s.n = c.fft_size;
  s.nsteps = nsteps;
  s.hop = c.scan_hop;
  s.total = c.scan_total_entries;
  s.step_lo = step_lo;
  s.own_steps = step_hi - step_lo;
  s.nhalo = nhalo;
  s.own_band_major = own_band_major;
  s.e_lo = elem_lo;
  s.e_hi = elem_hi;
  s.state = e->d_scan_state;
  s.first_pass = e->scan_passes == 0;
  s.b_max = e->b_max;
  s.b_min = e->b_min;
  s.base_is_raw = e->scan_base_is_raw;
  s.npasses = npasses;
  const int rows = std::min(npasses, KSA_HM_ROWS);       // only the last 128 passes of a batch reach the ring
  if (npasses > 1 || ranged) {
    // Fft.Avg after each of those passes: the waterfall row of a pass is built from it (K:696-697)
    if (!e->d_scan_avg_rows)
      HIP_OK(hipMalloc(reinterpret_cast<void**>(&e->d_scan_avg_rows), (size_t)KSA_HM_ROWS * s.total * 4));
    s.avg_rows = e->d_scan_avg_rows;
    s.avg_row0 = npasses - rows;
  }
  const int tb = 256;
  const int elems = elem_hi - elem_lo;
  if (elems > 0) hipLaunchKernelGGL(ksa::scan_stitch_kernel, dim3((elems + tb - 1) / tb), dim3(tb), 0, e->stream, s);
  const int g = c.scan_total_entries / c.scan_hm_width;
  if (ranged) {
    if (!e->d_scan_rows) HIP_OK(hipMalloc(reinterpret_cast<void**>(&e->d_scan_rows), (size_t)KSA_HM_ROWS * c.scan_hm_width * 4));
    hipLaunchKernelGGL(ksa::rowmax_rows_range_kernel, dim3(c.scan_hm_width, rows), dim3(64), 0, e->stream,
                       e->d_scan_avg_rows, e->d_scan_adj, c.scan_hm_width, g, elem_lo, elem_hi, e->d_scan_rows);
    HIP_OK(hipGetLastError());
    e->scan_rows = rows;
    e->scan_rows_passes = npasses;
    e->scan_passes += npasses;       // (the ring advances in ksa_scan_merge_rows_dev)
    return 0;
  }
  if (npasses == 1) {
    hipLaunchKernelGGL(ksa::rowmax_kernel, dim3((c.scan_hm_width + tb - 1) / tb), dim3(tb), 0, e->stream,
                       e->d_scan_state + (size_t)3 * s.total, e->d_scan_adj, c.scan_hm_width, g,
                       e->d_scan_hm + (size_t)e->scan_hm_index * c.scan_hm_width);
  } else {
    hipLaunchKernelGGL(ksa::rowmax_rows_kernel, dim3(c.scan_hm_width, rows), dim3(64), 0, e->stream,
                       e->d_scan_avg_rows, e->d_scan_adj, c.scan_hm_width, g, e->d_scan_hm,
                       (e->scan_hm_index + s.avg_row0) % KSA_HM_ROWS);
  }
  HIP_OK(hipGetLastError());
  e->scan_passes += npasses;
  e->scan_hm_index = (e->scan_hm_index + npasses) % KSA_HM_ROWS;  // K:732, once per pass
  return 0;
}

// Bands in front of step_lo that still cover elements from step_lo*hop on: ceil(N/hop) - 1, at most step_lo.
static int halo_bands(const ksa_config& c, int step_lo) { return std::min(step_lo, (c.fft_size + c.scan_hop - 1) / c.scan_hop - 1); }

int ksa_scan_stitch_range_dev(ksa_engine* e, const float* own_db_dev, int32_t own_band_major, const float* halo_db_dev,
                              int32_t nhalo, int32_t step_lo, int32_t step_hi, int32_t nsteps, int32_t npasses,
                              int32_t elem_lo, int32_t elem_hi) {
  if (!e) return fail("null engine");
  const ksa_config& c = e->cfg;
  if (!c.scan_total_entries) return fail("engine was created without scan geometry");
  if (nsteps < 1 || npasses < 1) return fail("nsteps and npasses must be >= 1");
  if (step_lo < 0 || step_hi < step_lo || step_hi > nsteps) return fail("bands [%d,%d) outside the pass of %d", step_lo, step_hi, nsteps);
  if (elem_lo < 0 || elem_hi < elem_lo || elem_hi > c.scan_total_entries)
    return fail("elements [%d,%d) outside the stitched range of %d", elem_lo, elem_hi, c.scan_total_entries);
  if (nhalo < 0 || nhalo > step_lo) return fail("nhalo %d outside 0..step_lo(%d)", nhalo, step_lo);
  if (elem_hi > elem_lo) {
    // every band that covers an owned element must be at hand: i0(elem_lo) >= step_lo - nhalo, i1(elem_hi-1) < step_hi
    const int n = c.fft_size, hop = c.scan_hop;
    const int i0 = elem_lo - n + 1 <= 0 ? 0 : (elem_lo - n + hop) / hop;
    const int i1 = std::min((elem_hi - 1) / hop, nsteps - 1);
    if (i0 <= i1 && (i0 < step_lo - nhalo || i1 >= step_hi))
      return fail("elements [%d,%d) are covered by bands %d..%d, at hand are %d..%d", elem_lo, elem_hi, i0, i1, step_lo - nhalo, step_hi - 1);
    if (step_hi > step_lo && !own_db_dev) return fail("null own_db_dev");
    if (nhalo > 0 && !halo_db_dev) return fail("null halo_db_dev");
  }
  const float* own = own_db_dev ? own_db_dev : e->d_scan_state;   // (an engine that owns no band reads nothing)
  DeviceGuard dev_guard;
  return scan_stitch(e, own, nsteps, npasses, true, halo_db_dev, nhalo, step_lo, step_hi, elem_lo, elem_hi, own_band_major != 0);
}

int ksa_scan_rows_dev(ksa_engine* e, float** rows_dev, int32_t* rows) {
  if (!e || !rows_dev || !rows) return fail("null argument");
  if (!e->d_scan_rows || e->scan_rows <= 0) return fail("no band-sharded batch pending (ksa_scan_stitch_range_dev first)");
  *rows_dev = e->d_scan_rows;
  *rows = e->scan_rows;
  return 0;
}

int ksa_scan_merge_rows_dev(ksa_engine* e, const float* gathered_dev, int32_t world, int32_t rows, int32_t npasses) {
  if (!e || !gathered_dev) return fail("null argument");
  const ksa_config& c = e->cfg;
  if (!c.scan_total_entries) return fail("engine was created without scan geometry");
  if (world < 1) return fail("world %d < 1", world);
  if (rows != e->scan_rows || npasses != e->scan_rows_passes)
    return fail("ksa_scan_merge_rows_dev: %d rows of %d passes pending, call says %d of %d", e->scan_rows, e->scan_rows_passes, rows, npasses);
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(c.device));
  const int cells = rows * c.scan_hm_width;
  hipLaunchKernelGGL(ksa::scan_merge_rows_kernel, dim3((cells + 255) / 256), dim3(256), 0, e->stream, gathered_dev, world,
                     rows, c.scan_hm_width, e->d_scan_hm, (e->scan_hm_index + npasses - rows) % KSA_HM_ROWS);
  HIP_OK(hipGetLastError());
  e->scan_hm_index = (e->scan_hm_index + npasses) % KSA_HM_ROWS;
  e->scan_rows = e->scan_rows_passes = 0;
  return 0;
}

// device-to-device copy issued on `s` (a stream of dst_dev): peer copy when the devices differ
static int copy_d2d(void* dst, int dst_dev, const void* src, int src_dev, size_t bytes, hipStream_t s) {
  if (!bytes) return 0;
  if (dst_dev == src_dev) HIP_OK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s));
  else HIP_OK(hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, s));
  return 0;
}

static int ensure_events(ksa_engine* e) {
  if (!e->ev_ready) HIP_OK(hipEventCreateWithFlags(&e->ev_ready, hipEventDisableTiming));
  if (!e->ev_copied) HIP_OK(hipEventCreateWithFlags(&e->ev_copied, hipEventDisableTiming));
  return 0;
}

// every engine -> every engine: engine i's stream receives block_of(j) of all j into its d_gather[j], behind the
// producers (ev_ready) ; ev_copied_i marks the end of i's copies so that no producer overwrites a block too early
static int gather_all(ksa_engine* const* h, int n, size_t nfloats, float* (*block_of)(ksa_engine*)) {
  for (int j = 0; j < n; ++j) {
    HIP_OK(hipSetDevice(h[j]->cfg.device));
    if (ensure_events(h[j])) return 1;
    HIP_OK(hipEventRecord(h[j]->ev_ready, h[j]->stream));
  }
  for (int i = 0; i < n; ++i) {
    ksa_engine* e = h[i];
    HIP_OK(hipSetDevice(e->cfg.device));
    if (ensure(&e->d_gather, &e->gather_cap, (size_t)n * nfloats)) return 1;
    for (int j = 0; j < n; ++j) {
      if (j != i) HIP_OK(hipStreamWaitEvent(e->stream, h[j]->ev_ready, 0));
      if (copy_d2d(e->d_gather + (size_t)j * nfloats, e->cfg.device, block_of(h[j]), h[j]->cfg.device, nfloats * 4, e->stream)) return 1;
    }
    HIP_OK(hipEventRecord(e->ev_copied, e->stream));
  }
  for (int i = 0; i < n; ++i) {
    HIP_OK(hipSetDevice(h[i]->cfg.device));
    for (int j = 0; j < n; ++j)
      if (j != i) HIP_OK(hipStreamWaitEvent(h[i]->stream, h[j]->ev_copied, 0));
  }
  return 0;
}

// Direct xGMI copies between the engines' GPUs where the hardware allows them (hipMemcpyPeerAsync works either way,
// through host staging otherwise).  Best effort: "already enabled" and "not supported" are not errors here.  Every
// ordered device pair is tried ONCE per process (a bit per pair), not on every multi-engine call.
static void enable_peer_access(ksa_engine* const* h, int n) {
  static std::mutex mu;
  static std::vector<unsigned char> tried;       // [a * ndev + b]
  static int ndev = 0;
  std::lock_guard<std::mutex> lock(mu);
  if (!ndev) {
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { ndev = 0; (void)hipGetLastError(); return; }
    tried.assign((size_t)ndev * ndev, 0);
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      const int a = h[i]->cfg.device, b = h[j]->cfg.device;
      if (a == b || a >= ndev || b >= ndev || tried[(size_t)a * ndev + b]) continue;
      tried[(size_t)a * ndev + b] = 1;
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, a, b) != hipSuccess || !can) { (void)hipGetLastError(); continue; }
      if (hipSetDevice(a) == hipSuccess) (void)hipDeviceEnablePeerAccess(b, 0);
      (void)hipGetLastError();
    }
}

static int check_handles(ksa_engine* const* h, int n) {
  if (!h || n < 1) return fail("need at least one engine handle");
  for (int i = 0; i < n; ++i) {
    if (!h[i]) return fail("engine handle %d is null", i);
    for (int j = 0; j < i; ++j) if (h[j] == h[i]) return fail("engine handle %d is handle %d again", i, j);
    const ksa_config &a = h[0]->cfg, &b = h[i]->cfg;
    if (a.fft_size != b.fft_size || a.hm_width != b.hm_width || a.scan_total_entries != b.scan_total_entries ||
        a.scan_hop != b.scan_hop || a.scan_hm_width != b.scan_hm_width)
      return fail("engine %d has a different geometry than engine 0", i);
  }
  enable_peer_access(h, n);
  return 0;
}

int ksa_allreduce_state(ksa_engine* const* handles, int32_t n, int32_t frames_per_rank, int32_t hm_index0) {
  DeviceGuard dev_guard;
  // everything is validated before the first copy or launch: a refusal leaves every engine as it was
  if (check_handles(handles, n)) return 1;
  if (frames_per_rank < 1) return fail("frames_per_rank %d < 1", frames_per_rank);
  if (hm_index0 < 0 || hm_index0 >= KSA_HM_ROWS) return fail("hm_index0 %d outside 0..127", hm_index0);
  for (int i = 0; i < n; ++i)
    if (handles[i]->pending_frames != frames_per_rank)
      return fail("engine %d has %d frames pending, frames_per_rank says %d", i, handles[i]->pending_frames, frames_per_rank);
  const size_t nfloats = 4 * (size_t)handles[0]->cfg.fft_size + (size_t)KSA_HM_ROWS * handles[0]->cfg.hm_width;
  if (gather_all(handles, n, nfloats, +[](ksa_engine* e) { return e->d_xchg; })) return 1;
  for (int i = 0; i < n; ++i)
    if (ksa_merge_gathered_dev(handles[i], handles[i]->d_gather, n, frames_per_rank, hm_index0)) return 1;
  return 0;
}

int ksa_scan_allstitch(ksa_engine* const* handles, int32_t n, float* const* own_db_dev, int32_t nsteps, int32_t npasses) {
  DeviceGuard dev_guard;
  if (check_handles(handles, n)) return 1;
  if (!own_db_dev) return fail("null own_db_dev");
  const ksa_config& c = handles[0]->cfg;
  if (!c.scan_total_entries) return fail("engines were created without scan geometry");
  if (nsteps < 1 || npasses < 1) return fail("nsteps and npasses must be >= 1");
  const size_t band = (size_t)npasses * c.fft_size;   // floats of one band over the batch
  const int reach = (c.fft_size + c.scan_hop - 1) / c.scan_hop - 1;   // bands in front of a band that still overlap it
  auto lo_of = [&](int r) { return (int)((long long)nsteps * r / n); };
  // 0. every pointer and range is checked before the first launch: a refusal at rank k must not leave ranks < k with
  //    their pass counters advanced and their state stitched while the ring is never merged
  for (int r = 0; r < n; ++r) {
    const int lo = lo_of(r), hi = lo_of(r + 1);
    if (hi > lo && !own_db_dev[r]) return fail("own_db_dev[%d] is null (rank %d owns bands %d..%d)", r, r, lo, hi - 1);
    if (handles[r]->scan_rows > 0) return fail("engine %d still holds unmerged partial rows of an earlier batch", r);
    const long long e_lo = (long long)lo * c.scan_hop;
    if (r < n - 1 && hi > lo && e_lo > c.scan_total_entries) return fail("rank %d's bands start past the stitched range", r);
  }
  // 1. every engine packs the bands its right neighbours need ([band][npasses][N]) behind its spectrum stage
  for (int r = 0; r < n; ++r) {
    ksa_engine* e = handles[r];
    const int lo = lo_of(r), hi = lo_of(r + 1), mine = hi - lo;
    HIP_OK(hipSetDevice(e->cfg.device));
    if (ensure_events(e)) return 1;
    const int keep = std::min(mine, reach);            // its last bands may be someone's halo
    if (keep > 0 && r + 1 < n) {
      if (ensure(&e->d_scan_send, &e->scan_send_cap, (size_t)keep * band)) return 1;
      for (int b = 0; b < keep; ++b)     // band hi-keep+b of every pass -> send[b][pass][N]
        HIP_OK(hipMemcpy2DAsync(e->d_scan_send + (size_t)b * band, (size_t)c.fft_size * 4,
                                own_db_dev[r] + (size_t)(mine - keep + b) * c.fft_size, (size_t)mine * c.fft_size * 4,
                                (size_t)c.fft_size * 4, (size_t)npasses, hipMemcpyDeviceToDevice, e->stream));
    }
    HIP_OK(hipEventRecord(e->ev_ready, e->stream));
  }
  // From here on engines are being modified: a failure must not leave partial rows behind that would make every later
  // ksa_scan_allstitch refuse ("still holds unmerged partial rows").
  auto abandon = [&]() { for (int r = 0; r < n; ++r) handles[r]->scan_rows = handles[r]->scan_rows_passes = 0; return 1; };
  // 2. halos: band j of rank r's halo comes from the rank that owns j
  for (int r = 0; r < n; ++r) {
    ksa_engine* e = handles[r];
    const int lo = lo_of(r), hi = lo_of(r + 1);
    const int nhalo = halo_bands(c, lo);
    HIP_OK(hipSetDevice(e->cfg.device));
    if (nhalo > 0 && ensure(&e->d_scan_halo, &e->scan_halo_cap, (size_t)nhalo * band)) return 1;
    for (int j = lo - nhalo; j < lo; ++j) {
      int src = r - 1;
      while (src > 0 && lo_of(src) > j) --src;
      ksa_engine* s = handles[src];
      const int shi = lo_of(src + 1), smine = shi - lo_of(src);
      const int skeep = std::min(smine, reach);
      const int b = j - (shi - skeep);                 // position of band j in src's send block
      if (b < 0) return fail("internal: band %d is not in rank %d's send block", j, src);
      HIP_OK(hipStreamWaitEvent(e->stream, s->ev_ready, 0));
      if (copy_d2d(e->d_scan_halo + (size_t)(j - (lo - nhalo)) * band, e->cfg.device, s->d_scan_send + (size_t)b * band,
                   s->cfg.device, band * 4, e->stream)) return 1;
    }
    const int elem_lo = lo * c.scan_hop, elem_hi = r == n - 1 ? c.scan_total_entries : std::min(c.scan_total_entries, hi * c.scan_hop);
    if (ksa_scan_stitch_range_dev(e, own_db_dev[r], 0, e->d_scan_halo, nhalo, lo, hi, nsteps, npasses, std::min(elem_lo, elem_hi), elem_hi)) return abandon();
  }
  // 3. partial waterfall rows: all-to-all copies, merged on every engine
  const int rows = std::min(npasses, KSA_HM_ROWS);
  const size_t nfloats = (size_t)rows * c.scan_hm_width;
  if (gather_all(handles, n, nfloats, +[](ksa_engine* e) { return e->d_scan_rows; })) return abandon();
  for (int i = 0; i < n; ++i)
    if (ksa_scan_merge_rows_dev(handles[i], handles[i]->d_gather, n, rows, npasses)) return abandon();
  return 0;
}

int ksa_scan_gather_state(ksa_engine* const* handles, int32_t n, int32_t nsteps, float* cur, float* max, float* min, float* avg) {
  DeviceGuard dev_guard;
  if (check_handles(handles, n)) return 1;
  const ksa_config& c = handles[0]->cfg;
  if (!c.scan_total_entries) return fail("engines were created without scan geometry");
  if (nsteps < 1) return fail("nsteps must be >= 1");
  float* dst[4] = {cur, max, min, avg};
  const size_t t = (size_t)c.scan_total_entries;
  for (int r = 0; r < n; ++r) {
    ksa_engine* e = handles[r];
    const long long lo = (long long)nsteps * r / n, hi = (long long)nsteps * (r + 1) / n;
    const size_t e_lo = std::min<size_t>(t, (size_t)lo * c.scan_hop), e_hi = r == n - 1 ? t : std::min<size_t>(t, (size_t)hi * c.scan_hop);
    HIP_OK(hipSetDevice(e->cfg.device));
    for (int k = 0; k < 4; ++k)
      if (dst[k] && e_hi > e_lo)
        HIP_OK(hipMemcpyAsync(dst[k] + e_lo, e->d_scan_state + k * t + e_lo, (e_hi - e_lo) * 4, hipMemcpyDeviceToHost, e->stream));
  }
  for (int r = 0; r < n; ++r) {
    HIP_OK(hipSetDevice(handles[r]->cfg.device));
    HIP_OK(hipStreamSynchronize(handles[r]->stream));
  }
  return 0;
}

static int scan_pass_host(ksa_engine* e, const void* iq_host, int fmt, int nsteps, const uint8_t* step_ok) {
  if (!e || !iq_host) return fail("null argument");
  if (!e->cfg.scan_total_entries) return fail("engine was created without scan geometry");
  if (nsteps < 1 || nsteps > e->cfg.max_frames) return fail("nsteps %d outside 1..max_frames(%d)", nsteps, e->cfg.max_frames);
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(e->cfg.device));
  const size_t bytes = (size_t)nsteps * e->cfg.full_size * sample_bytes(fmt);
  if (ensure(reinterpret_cast<unsigned char**>(&e->d_scan_stage), &e->scan_stage_cap, bytes)) return 1;
  HIP_OK(hipMemcpyAsync(e->d_scan_stage, iq_host, bytes, hipMemcpyHostToDevice, e->stream));
  if (ksa_scan_passes_dev(e, e->d_scan_stage, fmt, e->cfg.full_size, nsteps, 1, step_ok)) return 1;
  HIP_OK(hipStreamSynchronize(e->stream));
  return 0;
}

int ksa_scan_pass_c64(ksa_engine* e, const float* iq_host, int32_t nsteps, const uint8_t* step_ok) {
  return scan_pass_host(e, iq_host, KSA_FMT_C64, nsteps, step_ok);
}
int ksa_scan_pass_u8(ksa_engine* e, const uint8_t* iq_host, int32_t nsteps, const uint8_t* step_ok) {
  return scan_pass_host(e, iq_host, KSA_FMT_U8, nsteps, step_ok);
}

int ksa_host_alloc(void** out, int64_t bytes) {
  if (!out || bytes < 1) return fail("ksa_host_alloc: null pointer or size < 1");
  *out = nullptr;
  HIP_OK(hipHostMalloc(out, (size_t)bytes, hipHostMallocDefault));
  return 0;
}
int ksa_host_free(void* p) {
  if (p) HIP_OK(hipHostFree(p));
  return 0;
}

int ksa_scan_stitch_dev(ksa_engine* e, const float* step_db_dev, int32_t nsteps) {
  DeviceGuard dev_guard;
  return scan_stitch(e, step_db_dev, nsteps, 1);
}

int ksa_scan_stitch_passes_dev(ksa_engine* e, const float* step_db_dev, int32_t nsteps, int32_t npasses) {
  DeviceGuard dev_guard;
  return scan_stitch(e, step_db_dev, nsteps, npasses);
}

// Clip2MinAmp + LogNoGain spectra of `frames` capture blocks (K:640-641) into out_dev[frames][N]; a block whose
// step_ok entry is 0 is replaced by the dummy band: ones(fftSize) through the same two steps (K:637-641)
static int scan_spectra(ksa_engine* e, const void* iq_dev, int fmt, long long frame_stride, int frames, const uint8_t* step_ok,
                        float* out_dev) {
  if (run_spectrum(e, {iq_dev, fmt, frame_stride, frames}, KSA_OUT_DB_CLIP, out_dev, false, nullptr)) return 1;
  if (step_ok) {
    const float v = (float)(10.0 * std::log10(std::max(1.0, (double)e->cfg.min_amp)) - (double)e->cfg.gain);
    for (long long s = 0; s < frames; ++s)
      if (!step_ok[s] && fill(e, out_dev + (size_t)s * e->cfg.fft_size, e->cfg.fft_size, v)) return 1;
  }
  return 0;
}

int ksa_scan_spectra_dev(ksa_engine* e, const void* iq_dev, int32_t fmt, int64_t frame_stride, int32_t nframes,
                         const uint8_t* step_ok, float* out_dev) {
  if (!e || !iq_dev || !out_dev) return fail("null argument");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(e->cfg.device));
  return scan_spectra(e, iq_dev, fmt, frame_stride, nframes, step_ok, out_dev);
}

int ksa_scan_passes_dev(ksa_engine* e, const void* iq_dev, int32_t fmt, int64_t frame_stride, int32_t nsteps,
                        int32_t npasses, const uint8_t* step_ok) {
  if (!e || !iq_dev) return fail("null argument");
  if (!e->cfg.scan_total_entries) return fail("engine was created without scan geometry");
  if (nsteps < 1 || npasses < 1) return fail("nsteps and npasses must be >= 1");
  const long long frames = (long long)nsteps * npasses;
  if (frames > e->cfg.max_frames) return fail("%d passes x %d steps exceed max_frames %d", npasses, nsteps, e->cfg.max_frames);
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(e->cfg.device));
  if (scan_spectra(e, iq_dev, fmt, frame_stride, (int)frames, step_ok, e->d_frames)) return 1;
  return scan_stitch(e, e->d_frames, nsteps, npasses);
}

int ksa_scan_pass_dev(ksa_engine* e, const void* iq_dev, int32_t fmt, int64_t frame_stride, int32_t nsteps,
                      const uint8_t* step_ok) {
  return ksa_scan_passes_dev(e, iq_dev, fmt, frame_stride, nsteps, 1, step_ok);
}

int ksa_scan_read_state(ksa_engine* e, float* cur, float* max, float* min, float* avg, float* hm, int32_t* hm_index,
                        int64_t* passes) {
  if (!e) return fail("null engine");
  if (!e->cfg.scan_total_entries) return fail("engine was created without scan geometry");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(e->cfg.device));
  const size_t t = (size_t)e->cfg.scan_total_entries;
  float* dst[4] = {cur, max, min, avg};
  for (int i = 0; i < 4; ++i)
    if (dst[i]) HIP_OK(hipMemcpyAsync(dst[i], e->d_scan_state + i * t, t * 4, hipMemcpyDeviceToHost, e->stream));
  if (hm) HIP_OK(hipMemcpyAsync(hm, e->d_scan_hm, (size_t)KSA_HM_ROWS * e->cfg.scan_hm_width * 4, hipMemcpyDeviceToHost, e->stream));
  HIP_OK(hipStreamSynchronize(e->stream));
  if (hm_index) *hm_index = e->scan_hm_index;
  if (passes) *passes = e->scan_passes;
  return 0;
}

int ksa_scan_state_dev(ksa_engine* e, float** state_dev, float** hm_ring_dev) {
  if (!e) return fail("null engine");
  if (state_dev) *state_dev = e->d_scan_state;
  if (hm_ring_dev) *hm_ring_dev = e->d_scan_hm;
  return 0;
}

int ksa_scan_set_base_is_raw(ksa_engine* e, int32_t on) {
  if (!e) return fail("null engine");
  e->scan_base_is_raw = on != 0;
  return 0;
}

int ksa_scan_reset(ksa_engine* e) {
  if (!e) return fail("null engine");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(e->cfg.device));
  return scan_reset(e);
}

static int levels_to_scratch(ksa_engine* e, int scan, int mode, int cells) {
  if (mode < 0 || mode > 2) return fail("levels mode %d (0 AVG, 1 MAX, 2 MIN)", mode);
  const int n = scan ? e->cfg.scan_total_entries : e->cfg.fft_size;
  if (scan && !n) return fail("engine was created without scan geometry");
  if (cells < 1 || n % cells) return fail("cells %d must divide %d", cells, n);
  HIP_OK(hipSetDevice(e->cfg.device));     // (the exported caller holds the DeviceGuard)
  if (!e->d_levels || e->levels_cap < cells) {
    if (e->d_levels) hipFree(e->d_levels);
    e->d_levels = nullptr;
    HIP_OK(hipMalloc(reinterpret_cast<void**>(&e->d_levels), (size_t)4 * cells * 4));
    e->levels_cap = cells;
  }
  const int tb = 128;
  hipLaunchKernelGGL(ksa::levels_kernel, dim3((cells + tb - 1) / tb, 4), dim3(tb), 0, e->stream,
                     scan ? e->d_scan_state : e->d_state, scan ? e->d_scan_adj : e->d_adj, n, cells, mode, e->d_levels);
  HIP_OK(hipGetLastError());
  return 0;
}

int ksa_read_levels(ksa_engine* e, int32_t scan, int32_t mode, int32_t cells, float* out_host) {
  if (!e || !out_host) return fail("null argument");
  DeviceGuard dev_guard;
  if (levels_to_scratch(e, scan, mode, cells)) return 1;
  HIP_OK(hipMemcpyAsync(out_host, e->d_levels, (size_t)4 * cells * 4, hipMemcpyDeviceToHost, e->stream));
  HIP_OK(hipStreamSynchronize(e->stream));
  return 0;
}

int ksa_read_highs(ksa_engine* e, int32_t scan, int32_t mode, int32_t cells, int32_t curve, double min_sep_cells,
                   int32_t count, int32_t* idx_host, float* lvl_host, int32_t* found) {
  if (!e || !idx_host || !lvl_host || !found) return fail("null argument");
  if (curve < 0 || curve > 3) return fail("curve %d (0 cur, 1 max, 2 min, 3 avg)", curve);
  if (count < 1 || count > ksa::HIGHS_MAX) return fail("marker count %d outside 1..%d", count, ksa::HIGHS_MAX);
  if (!(min_sep_cells >= 0.0)) return fail("min_sep_cells must be >= 0");
  DeviceGuard dev_guard;
  if (levels_to_scratch(e, scan, mode, cells)) return 1;
  if (!e->d_highs) HIP_OK(hipMalloc(reinterpret_cast<void**>(&e->d_highs), (2 * ksa::HIGHS_MAX + 1) * 4));
  ksa::HighsParams h{};
  h.lv = e->d_levels + (size_t)curve * cells;
  h.cells = cells;
  h.min_sep = min_sep_cells;
  h.count = count;
  h.idx = e->d_highs;
  h.lvl = reinterpret_cast<float*>(e->d_highs + ksa::HIGHS_MAX);
  h.found = e->d_highs + 2 * ksa::HIGHS_MAX;
  hipLaunchKernelGGL(ksa::highs_kernel, dim3(1), dim3(1024), 0, e->stream, h);
  HIP_OK(hipGetLastError());
  int host[2 * ksa::HIGHS_MAX + 1];
  HIP_OK(hipMemcpyAsync(host, e->d_highs, sizeof host, hipMemcpyDeviceToHost, e->stream));
  HIP_OK(hipStreamSynchronize(e->stream));
  *found = host[2 * ksa::HIGHS_MAX];
  for (int i = 0; i < *found; ++i) {
    idx_host[i] = host[i];
    memcpy(&lvl_host[i], &host[ksa::HIGHS_MAX + i], 4);
  }
  return 0;
}

// rows [row0, row0 + nrows) (mod 128) of a waterfall ring -> host
static int copy_ring_rows(ksa_engine* e, int scan, int row0, int nrows, float* out_host) {
  const float* ring = scan ? e->d_scan_hm : e->d_hm;
  const int w = scan ? e->cfg.scan_hm_width : e->cfg.hm_width;
  if (!ring || w < 1) return fail("engine has no %s waterfall", scan ? "scan" : "zeroSpan");
  if (row0 < 0 || row0 >= KSA_HM_ROWS || nrows < 0 || nrows > KSA_HM_ROWS) return fail("ring rows [%d,+%d) outside 0..127", row0, nrows);
  const int first = std::min(nrows, KSA_HM_ROWS - row0);
  if (first > 0) HIP_OK(hipMemcpyAsync(out_host, ring + (size_t)row0 * w, (size_t)first * w * 4, hipMemcpyDeviceToHost, e->stream));
  if (nrows > first)
    HIP_OK(hipMemcpyAsync(out_host + (size_t)first * w, ring, (size_t)(nrows - first) * w * 4, hipMemcpyDeviceToHost, e->stream));
  return 0;
}

int ksa_read_hm_rows(ksa_engine* e, int32_t scan, int32_t row0, int32_t nrows, float* out_host) {
  if (!e || !out_host) return fail("null argument");
  if (scan && !e->cfg.scan_total_entries) return fail("engine was created without scan geometry");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(e->cfg.device));
  if (copy_ring_rows(e, scan, row0, nrows, out_host)) return 1;
  HIP_OK(hipStreamSynchronize(e->stream));
  return 0;
}

int ksa_read_view(ksa_engine* e, int32_t scan, int32_t mode, int32_t cells, float* levels_host, int32_t curve,
                  double min_sep_cells, int32_t count, int32_t* idx_host, float* lvl_host, int32_t* found,
                  int32_t hm_rows, float* hm_rows_host, int32_t* hm_index) {
  if (!e || !levels_host) return fail("null argument");
  if (count > 0 && (!idx_host || !lvl_host || !found)) return fail("null marker outputs");
  if (count < 0 || count > ksa::HIGHS_MAX) return fail("marker count %d outside 0..%d", count, ksa::HIGHS_MAX);
  if (count > 0 && (curve < 0 || curve > 3)) return fail("curve %d (0 cur, 1 max, 2 min, 3 avg)", curve);
  if (count > 0 && !(min_sep_cells >= 0.0)) return fail("min_sep_cells must be >= 0");
  if (hm_rows < 0 || hm_rows > KSA_HM_ROWS || (hm_rows > 0 && !hm_rows_host)) return fail("hm_rows %d outside 0..128 or null buffer", hm_rows);
  if (scan && !e->cfg.scan_total_entries) return fail("engine was created without scan geometry");
  if (hm_rows > 0 && (!(scan ? e->d_scan_hm : e->d_hm) || (scan ? e->cfg.scan_hm_width : e->cfg.hm_width) < 1))
    return fail("engine has no %s waterfall", scan ? "scan" : "zeroSpan");
  if (found) *found = 0;
  DeviceGuard dev_guard;
  if (levels_to_scratch(e, scan, mode, cells)) return 1;       // (selects the device; nothing is enqueued towards the host yet)
  // From the first asynchronous copy on, every exit synchronises the stream: the copies target caller buffers and a stack
  // array that must not be written after this function has returned.
  struct SyncOnExit {
    hipStream_t s; bool armed = true;
    ~SyncOnExit() { if (armed) (void)hipStreamSynchronize(s); }
  } drain{e->stream};
  HIP_OK(hipMemcpyAsync(levels_host, e->d_levels, (size_t)4 * cells * 4, hipMemcpyDeviceToHost, e->stream));
  int host[2 * ksa::HIGHS_MAX + 1];
  if (count > 0) {
    if (!e->d_highs) HIP_OK(hipMalloc(reinterpret_cast<void**>(&e->d_highs), (2 * ksa::HIGHS_MAX + 1) * 4));
    ksa::HighsParams h{};
    h.lv = e->d_levels + (size_t)curve * cells;
    h.cells = cells;
    h.min_sep = min_sep_cells;
    h.count = count;
    h.idx = e->d_highs;
    h.lvl = reinterpret_cast<float*>(e->d_highs + ksa::HIGHS_MAX);
    h.found = e->d_highs + 2 * ksa::HIGHS_MAX;
    hipLaunchKernelGGL(ksa::highs_kernel, dim3(1), dim3(1024), 0, e->stream, h);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(host, e->d_highs, sizeof host, hipMemcpyDeviceToHost, e->stream));
  }
  const int idx = scan ? e->scan_hm_index : e->hm_index;       // the ring position AFTER the newest row
  if (hm_rows > 0 && copy_ring_rows(e, scan, ((idx - hm_rows) % KSA_HM_ROWS + KSA_HM_ROWS) % KSA_HM_ROWS, hm_rows, hm_rows_host)) return 1;
  drain.armed = false;
  HIP_OK(hipStreamSynchronize(e->stream));
  if (count > 0) {
    *found = host[2 * ksa::HIGHS_MAX];
    for (int i = 0; i < *found; ++i) {
      idx_host[i] = host[i];
      memcpy(&lvl_host[i], &host[ksa::HIGHS_MAX + i], 4);
    }
  }
  if (hm_index) *hm_index = idx;
  return 0;
}

int ksa_prof_enable(ksa_engine* e, int32_t on) {
  if (!e) return fail("null engine");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(e->cfg.device));
  for (auto& pr : e->prof_events) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
  e->prof_events.clear();
  e->prof = on != 0;
  if (on) {
    const size_t bytes = (size_t)ksa::CLK_SLOTS * 2 * ksa::CLK_KEYS * 2 * sizeof(unsigned long long);
    if (!e->d_clk) HIP_OK(hipMalloc(reinterpret_cast<void**>(&e->d_clk), bytes));
    HIP_OK(hipMemsetAsync(e->d_clk, 0, bytes, e->stream));
    e->clk_launches = 0;
  }
  return 0;
}

int ksa_prof_read(ksa_engine* e, double* spectrum_ms, int64_t* launches) {
  if (!e) return fail("null engine");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(e->cfg.device));
  HIP_OK(hipStreamSynchronize(e->stream));
  double ms = 0;
  for (auto& pr : e->prof_events) {
    float t = 0;
    HIP_OK(hipEventElapsedTime(&t, pr.first, pr.second));
    ms += t;
  }
  if (spectrum_ms) *spectrum_ms = ms;
  if (launches) *launches = (int64_t)e->prof_events.size();
  return 0;
}

int ksa_prof_clock(ksa_engine* e, double* shader_ghz, double* ghz_min, double* ghz_max, int64_t* samples) {
  if (!e || !shader_ghz) return fail("null argument");
  *shader_ghz = 0.0;
  if (ghz_min) *ghz_min = 0.0;
  if (ghz_max) *ghz_max = 0.0;
  if (samples) *samples = 0;
  if (!e->d_clk) return fail("ksa_prof_clock: profiling was never enabled on this engine");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(e->cfg.device));
  HIP_OK(hipStreamSynchronize(e->stream));
  const size_t per = (size_t)2 * ksa::CLK_KEYS * 2;      // qwords per profiled launch
  std::vector<unsigned long long> h((size_t)ksa::CLK_SLOTS * per);
  HIP_OK(hipMemcpy(h.data(), e->d_clk, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  std::vector<double> ghz;
  for (int slot = 0; slot < ksa::CLK_SLOTS; ++slot)
    for (int key = 0; key < ksa::CLK_KEYS; ++key) {
      const unsigned long long* b0 = &h[slot * per + (size_t)key * 2];
      const unsigned long long* b1 = b0 + (size_t)ksa::CLK_KEYS * 2;
      const unsigned long long c0 = b0[0], r0 = b0[1], c1 = b1[0], r1 = b1[1];
      if (r0 && r1 > r0 && c1 > c0 && r1 - r0 >= 1000)    // this CU was stamped at both ends, >= 10 us apart (100 MHz ticks)
        ghz.push_back((double)(c1 - c0) / (double)(r1 - r0) * 0.1);
    }
  if (samples) *samples = (int64_t)ghz.size();
  if (ghz.empty()) return 0;
  std::sort(ghz.begin(), ghz.end());
  *shader_ghz = ghz[ghz.size() / 2];
  if (ghz_min) *ghz_min = ghz.front();
  if (ghz_max) *ghz_max = ghz.back();
  return 0;
}

int ksa_kernel_info(ksa_engine* e, int32_t* threads, int32_t* lds_bytes, int32_t* vgprs, int32_t* grid, int32_t* path) {
  if (!e) return fail("null engine");
  if (threads) *threads = e->threads;
  if (lds_bytes) *lds_bytes = e->lds_bytes;
  if (vgprs) *vgprs = e->vgprs;
  if (grid) *grid = e->num_cu * e->blocks_per_cu;
  if (path) *path = (e->path == 0 && e->plan32) ? 3 : (e->path == 0 && e->pair_ok) ? 4 : (e->path == 0 && e->k64_ok) ? 5 : e->path;
  if (e->path == 0 && e->k64_ok) {            // what complex64 input runs
    if (lds_bytes) *lds_bytes = ksa::Plan64::LDS_BYTES;
    if (vgprs) *vgprs = e->k64_vgprs;
    if (grid) *grid = e->num_cu * e->k64_bpc;
  }
  if (e->path == 0 && e->pair_ok) {           // what large batches run
    if (lds_bytes) *lds_bytes = e->pair_lds;
    if (vgprs) *vgprs = e->pair_vgprs;
    if (grid) *grid = e->num_cu * e->pair_bpc;
  }
  return 0;
}

}  // extern "C"
