// libksa_corr: host layer of include/ksa_corr.h (validation, launch planning, stream state, staging); kernels in
// kcr_kernels.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/ksa_corr.h"
#include "kcr_kernels.hpp"
#include "../csrc_shared/ksa_host.hpp"

static_assert(sizeof(kcr_event) == 4 * ksa::corr::EVENT_WORDS, "kcr_event and the kernels' record are one layout");
static_assert(KCR_FMT_C64 == ksa::iq::FMT_C64 && KCR_FMT_U8 == ksa::iq::FMT_U8 && KCR_FMT_S8 == ksa::iq::FMT_S8 &&
                  KCR_FMT_S16 == ksa::iq::FMT_S16,
              "the formats of the header are the kernels'");

namespace {

constexpr int WG_PER_CU = 16;                   // the grid's cap: workgroups per compute unit; a workgroup walks the tiles beyond

// W = 256 R lags per workgroup, R a function of Q; the span of W + K - 1 samples, rounded up to whole rows, as complex64
struct Plan {
  int per_thread = 0, tile_out = 0, lds_bytes = 0;
};

Plan plan_for(int K, int Q) {
  Plan p;
  p.per_thread = ksa::corr::lags_per_thread(Q);
  p.tile_out = ksa::corr::THREADS * p.per_thread;
  p.lds_bytes = p.per_thread * ksa::corr::row_len(K, p.per_thread) * 8;
  return p;
}

const void* corr_fn(int Q) {
  using namespace ksa::corr;
  switch (Q) {
    case 1: return reinterpret_cast<const void*>(corr_kernel<1>);
    case 2: return reinterpret_cast<const void*>(corr_kernel<2>);
    case 3: return reinterpret_cast<const void*>(corr_kernel<3>);
    case 4: return reinterpret_cast<const void*>(corr_kernel<4>);
    case 5: return reinterpret_cast<const void*>(corr_kernel<5>);
    case 6: return reinterpret_cast<const void*>(corr_kernel<6>);
    case 7: return reinterpret_cast<const void*>(corr_kernel<7>);
    default: return reinterpret_cast<const void*>(corr_kernel<8>);
  }
}

}  // namespace

struct kcr_corr {
  int device = 0, fmt = 0, K = 1, Q = 1, G = 1, capacity = 0, cus = 1, last_grid = 0, cur = 0;
  bool lost = false;                            // a stream call failed between its launches: kcr_reset starts anew
  bool flushed = false;
  float u8_offset = 127.5f, u8_inv_scale = 1.f / 127.5f, threshold = 0.5f, min_energy = 0.f;
  long long max_in = 0, work_lags = 0, chunks_max = 0;
  long long n_in = 0, decided = 0;              // samples in; lags decided
  Plan plan;
  const void* kernel = nullptr;
  float* tmpl = nullptr;                        // device [Q][K][4]: (cr, -ci, ci, cr)
  float* ec = nullptr;                          // device [Q]
  float2* hist[2] = {nullptr, nullptr};         // device, the stream's last K + 2G - 1 samples and the ones being written
  float* rho = nullptr;                         // device work [Q * work_lags]
  float2* r = nullptr;                          // device work [Q * work_lags]
  unsigned* events = nullptr;                   // device [capacity] records
  long long* totals = nullptr;                  // device [2]: events_total, its snapshot
  int* cnt = nullptr;                           // device [chunks_max]
  long long* off = nullptr;                     // device [chunks_max]
  long long* block_sums = nullptr;              // device [chunks_max / SCAN_THREADS + 1]
  char* stage = nullptr;                        // kcr_process: the call's input
  long long stage_bytes = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_stream = nullptr;
};

namespace {

int in_bytes(const kcr_corr* h) { return iq_sample_bytes(h->fmt); }
int keep_max(const kcr_corr* h) { return h->K + 2 * h->G - 1; }
long long lags_after(const kcr_corr* h, long long seen) { return std::max(0ll, seen - h->K + 1); }
size_t events_bytes(const kcr_corr* h) { return (size_t)h->capacity * sizeof(kcr_event); }

void free_all(kcr_corr* h) {
  if (h->ev_stream) (void)hipEventDestroy(h->ev_stream);
  free_device({h->tmpl, h->ec, h->hist[0], h->hist[1], h->rho, h->r, h->events, h->totals, h->cnt, h->off, h->block_sums, h->stage});
  delete h;
}

int check_params(float threshold, float min_energy) {
  if (!(std::isfinite(threshold) && threshold > 0.f && threshold <= 1.f))
    return fail("threshold %g is not a finite value in (0, 1]", (double)threshold);
  if (!(std::isfinite(min_energy) && min_energy >= 0.f)) return fail("min_energy %g is not a finite value >= 0", (double)min_energy);
  return 0;
}

// the templates' own rules, shared by kcr_create and kcr_set_templates; ec[q] in float64, rounded once
int check_templates(int K, int Q, const float* t, float* ec) {
  if (!t) return fail("null templates pointer");
  for (int q = 0; q < Q; ++q) {
    double sum = 0.0;
    for (int k = 0; k < K; ++k) {
      const float re = t[2 * ((size_t)q * K + k)], im = t[2 * ((size_t)q * K + k) + 1];
      if (!std::isfinite(re) || !std::isfinite(im)) return fail("template %d has a non-finite value at index %d", q, k);
      sum += (double)re * re + (double)im * im;
    }
    const float e = (float)sum;
    if (!(e > 0.f)) return fail("template %d has zero energy", q);
    if (!std::isfinite(e)) return fail("template %d has an energy beyond float32", q);
    ec[q] = e;
  }
  return 0;
}

// what the kernel's two packed multiply-adds of a tap take: (cr, -ci) beside xr, (ci, cr) beside xi
std::vector<float> packed(int K, int Q, const float* t) {
  std::vector<float> g((size_t)Q * K * 4);
  for (size_t i = 0; i < (size_t)Q * K; ++i) {
    g[4 * i] = t[2 * i];
    g[4 * i + 1] = -t[2 * i + 1];
    g[4 * i + 2] = t[2 * i + 1];
    g[4 * i + 3] = t[2 * i];
  }
  return g;
}

ksa::corr::Args base_args(const kcr_corr* h) {
  ksa::corr::Args a{};
  a.tmpl = h->tmpl;
  a.ec = h->ec;
  a.rho = h->rho;
  a.r = h->r;
  a.fmt = h->fmt;
  a.u8_offset = h->u8_offset;
  a.u8_inv_scale = h->u8_inv_scale;
  a.K = h->K;
  a.min_energy = h->min_energy;
  return a;
}

int launch_corr(kcr_corr* h, ksa::corr::Args& a, long long nblocks) {
  a.tiles = ceil_div(a.nl, h->plan.tile_out);
  a.total = a.tiles * nblocks;
  const long long grid = std::min(a.total, (long long)h->cus * WG_PER_CU);
  void* params[] = {&a};
  HIP_OK(hipLaunchKernel(h->kernel, dim3((unsigned)grid), dim3(ksa::corr::THREADS), params, (size_t)h->plan.lds_bytes, h->stream));
  h->last_grid = (int)grid;
  return 0;
}

// the peaks among work lags [d_a, d_a + nd) of every block, appended in (block, pos, templ) order
int launch_pick(kcr_corr* h, long long nblocks, int nl, int d_a, int nd, long long pos_base, bool stream) {
  using namespace ksa::corr;
  PickArgs p{};
  p.rho = h->rho;
  p.r = h->r;
  p.cnt = h->cnt;
  p.off = h->off;
  p.events = h->events;
  p.items = nblocks * nd * h->Q;
  p.pos_base = pos_base;
  p.stream = stream ? 1 : 0;
  p.nl = nl;
  p.d_a = d_a;
  p.nd = nd;
  p.Q = h->Q;
  p.G = h->G;
  p.capacity = h->capacity;
  p.threshold = h->threshold;
  const long long chunks = ceil_div(p.items, CHUNK);
  if (chunks < 1) return 0;
  if (chunks > h->chunks_max) return fail("internal: %lld chunks exceed the %lld planned", chunks, h->chunks_max);
  ScanArgs s{};
  s.cnt = h->cnt;
  s.n = (int)chunks;
  s.block_sums = h->block_sums;
  s.total = h->totals;
  s.snapshot = h->totals + 1;
  s.off = h->off;
  const unsigned blocks = (unsigned)ceil_div(chunks, SCAN_THREADS);
  hipLaunchKernelGGL(pick_kernel<false>, dim3((unsigned)chunks), dim3(THREADS), 0, h->stream, p);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(sum_kernel, dim3(blocks), dim3(SCAN_THREADS), 0, h->stream, s);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(offset_kernel, dim3(blocks), dim3(SCAN_THREADS), 0, h->stream, s);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(pick_kernel<true>, dim3((unsigned)chunks), dim3(THREADS), 0, h->stream, p);
  HIP_OK(hipGetLastError());
  return 0;
}

// The next n samples of the stream at in (device-visible); final: decide every lag that exists (kcr_flush, n = 0).
// Work lag 0 is stream lag A = max(0, decided - G): the lags from there to the last one that exists are formed anew from the
// history and the call's samples, which is what makes the cut of the stream invisible.
int stream_call(kcr_corr* h, const void* in, long long n, float* metric, float2* corr, long long out_stride, bool final) {
  const long long N0 = h->n_in, N1 = N0 + n, L0 = lags_after(h, N0), L1 = lags_after(h, N1);
  const long long D0 = h->decided, D1 = final ? L1 : std::max(0ll, L1 - h->G);
  const long long A = std::max(0ll, D0 - h->G);
  const int hist_len = (int)std::min<long long>(N0, keep_max(h));
  ksa::corr::Args a = base_args(h);
  a.in = in;
  a.hist = h->hist[h->cur];
  a.raw_len = (int)n;
  a.hist_len = hist_len;
  a.metric_out = metric;
  a.corr_out = corr;
  a.out_stride = out_stride;
  bool launched = false;
  int rc = 0;
  if (L1 > L0 || D1 > D0) {
    a.v0 = (int)(A - (N0 - hist_len));          // >= 0: the history reaches back to lag A
    a.nl = (int)(L1 - A);                       // <= n + 2G
    a.dense_first = (int)(L0 - A);
    if (a.v0 < 0 || a.nl > h->work_lags) return fail("internal: the stream state does not cover lag %lld", A);
    rc = launch_corr(h, a, 1);
    launched = rc == 0;
    if (!rc && D1 > D0) rc = launch_pick(h, 1, a.nl, (int)(D0 - A), (int)(D1 - D0), A, true);
  }
  if (!rc && n > 0) {
    const int keep = (int)std::min<long long>(N1, keep_max(h));
    const int shift = (int)(hist_len + n - keep);
    float2* next = h->hist[h->cur ^ 1];
    hipLaunchKernelGGL(ksa::corr::history_kernel, dim3((unsigned)ceil_div(keep, ksa::corr::THREADS)), dim3(ksa::corr::THREADS), 0,
                       h->stream, a, next, keep, shift);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) rc = fail("launching the history kernel failed: %s", hipGetErrorString(e));
  }
  if (rc) {                                     // outputs or events may be written, history and counts are not
    h->lost = h->lost || launched;
    return rc;
  }
  if (n > 0) h->cur ^= 1;
  h->n_in = N1;
  h->decided = D1;
  return 0;
}

int check_stream_args(kcr_corr* h, const void* in, int64_t n_in, const void* metric, const void* corr, int64_t out_stride,
                      int64_t* lags) {
  if (!h) return fail("null correlator object");
  if (n_in < 0) return fail("n_in %lld must be >= 0", (long long)n_in);
  if (n_in > h->max_in) return fail("n_in %lld exceeds max_in %lld", (long long)n_in, h->max_in);
  if (n_in > 0 && !in) return fail("null input pointer");
  if (int rc = check_iq_aligned(in, in_bytes(h))) return rc;
  if (h->flushed) return fail("the stream was flushed; kcr_reset starts a new stream");
  if (h->lost) return fail("the stream state was lost when an earlier call failed after its first launch; kcr_reset starts a new stream");
  if (n_in > KCR_MAX_POSITION - h->n_in)
    return fail("n_in %lld would take the stream from %lld samples past 2^52", (long long)n_in, h->n_in);
  *lags = lags_after(h, h->n_in + n_in) - lags_after(h, h->n_in);
  if ((metric || corr) && out_stride < *lags)
    return fail("out_stride %lld is shorter than the %lld lags of the call", (long long)out_stride, (long long)*lags);
  return 0;
}

}  // namespace

extern "C" {

int kcr_abi_version(void) { return KCR_ABI_VERSION; }
const char* kcr_last_error(void) { return g_err.c_str(); }

int kcr_create(int32_t device, int32_t fmt, float u8_offset, float u8_scale, int32_t K, int32_t Q, const float* templates_host,
               float threshold, float min_energy, int32_t guard, int32_t capacity, int64_t max_in, kcr_corr** out) {
  if (!out) return fail("null out pointer");
  *out = nullptr;
  if (check_iq_format(fmt)) return 1;
  if (K < 1 || K > KCR_MAX_K) return fail("K %d outside 1..%d", K, KCR_MAX_K);
  if (Q < 1 || Q > KCR_MAX_Q) return fail("Q %d outside 1..%d", Q, KCR_MAX_Q);
  if (Q * K > KCR_MAX_TEMPLATE_VALUES) return fail("Q x K = %d template values exceed %d", Q * K, KCR_MAX_TEMPLATE_VALUES);
  float ec[KCR_MAX_Q];
  if (int rc = check_templates(K, Q, templates_host, ec)) return rc;
  if (int rc = check_params(threshold, min_energy)) return rc;
  if (guard < 1 || guard > KCR_MAX_GUARD) return fail("guard %d outside 1..%d", guard, KCR_MAX_GUARD);
  if (capacity < 1 || capacity > KCR_MAX_CAPACITY) return fail("event capacity %d outside 1..%d", capacity, KCR_MAX_CAPACITY);
  if (max_in < 1 || max_in > KCR_MAX_IN) return fail("max_in %lld outside 1..%d", (long long)max_in, KCR_MAX_IN);
  if (check_u8_scaling(fmt, u8_offset, u8_scale)) return 1;
  if (check_device(device)) return 1;

  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(device));
  kcr_corr* h = new kcr_corr;
  h->device = device; h->fmt = fmt; h->K = K; h->Q = Q; h->G = guard; h->capacity = capacity; h->max_in = max_in;
  h->threshold = threshold; h->min_energy = min_energy;
  if (fmt == KCR_FMT_U8) { h->u8_offset = u8_offset; h->u8_inv_scale = 1.0f / u8_scale; }
  h->work_lags = max_in + 2 * guard;
  h->chunks_max = ceil_div(h->work_lags * Q, ksa::corr::CHUNK);
  h->plan = plan_for(K, Q);
  h->kernel = corr_fn(Q);
  const std::vector<float> table = packed(K, Q, templates_host);
  int rc = 0;
  do {
    if ((rc = cu_count(device, &h->cus))) break;
    const size_t tb = table.size() * 4, hb = (size_t)keep_max(h) * 8, wl = (size_t)h->work_lags * Q;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->tmpl), tb);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->ec), (size_t)Q * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->hist[0]), hb);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->hist[1]), hb);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->rho), wl * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->r), wl * 8);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->events), events_bytes(h));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->totals), 16);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->cnt), (size_t)h->chunks_max * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->off), (size_t)h->chunks_max * sizeof(long long));
    if (e == hipSuccess)
      e = hipMalloc(reinterpret_cast<void**>(&h->block_sums), (size_t)(h->chunks_max / ksa::corr::SCAN_THREADS + 1) * sizeof(long long));
    if (e != hipSuccess) { rc = fail("hipMalloc of the correlator's device memory failed: %s", hipGetErrorString(e)); break; }
    e = hipMemsetAsync(h->events, 0, events_bytes(h), h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->totals, 0, 16, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h->tmpl, table.data(), tb, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h->ec, ec, (size_t)Q * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { rc = fail("filling the correlator's device memory failed: %s", hipGetErrorString(e)); break; }
  } while (0);
  if (rc) {
    free_all(h);
    return rc;
  }
  *out = h;
  return 0;
}

void kcr_destroy(kcr_corr* h) {
  if (!h) return;
  DeviceGuard dev_guard;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  free_all(h);
}

int kcr_set_stream(kcr_corr* h, void* hip_stream) {
  if (!h) return fail("null correlator object");
  return hand_over_stream(h->device, &h->stream, &h->ev_stream, hip_stream);
}

int kcr_synchronize(kcr_corr* h) {
  if (!h) return fail("null correlator object");
  return synchronize_on(h->device, h->stream);
}

int kcr_out_count(kcr_corr* h, int64_t n_in, int64_t* n_lags) {
  if (!h) return fail("null correlator object");
  if (!n_lags) return fail("null n_lags pointer");
  if (n_in < 0) return fail("n_in %lld must be >= 0", (long long)n_in);
  if (n_in > KCR_MAX_POSITION - h->n_in)
    return fail("n_in %lld would take the stream from %lld samples past 2^52", (long long)n_in, h->n_in);
  *n_lags = lags_after(h, h->n_in + n_in) - lags_after(h, h->n_in);
  return 0;
}

int kcr_process_dev(kcr_corr* h, const void* iq_dev, int64_t n_in, float* metric_dev, void* corr_dev, int64_t out_stride,
                    int64_t* n_lags) {
  int64_t lags = 0;
  if (int rc = check_stream_args(h, iq_dev, n_in, metric_dev, corr_dev, out_stride, &lags)) return rc;
  if (n_lags) *n_lags = lags;
  if (n_in == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  return stream_call(h, iq_dev, n_in, metric_dev, static_cast<float2*>(corr_dev), out_stride, false);
}

int kcr_process(kcr_corr* h, const void* iq_host, int64_t n_in, float* metric_host, void* corr_host, int64_t out_stride,
                int64_t* n_lags) {
  int64_t lags = 0;
  if (int rc = check_stream_args(h, iq_host, n_in, metric_host, corr_host, out_stride, &lags)) return rc;
  if (n_lags) *n_lags = lags;
  if (n_in == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  const long long bytes = (long long)n_in * in_bytes(h);
  if (int rc = grow_device(&h->stage, &h->stage_bytes, bytes, h->stream)) return rc;
  HIP_OK(hipMemcpyAsync(h->stage, iq_host, (size_t)bytes, hipMemcpyHostToDevice, h->stream));
  // work lag 0 of this call is stream lag A, the call's first completed lag is work lag first; the work rows have nl lags
  const long long L0 = lags_after(h, h->n_in), L1 = L0 + lags, A = std::max(0ll, h->decided - h->G);
  const long long first = L0 - A, nl = L1 - A;
  if (int rc = stream_call(h, h->stage, n_in, nullptr, nullptr, 0, false)) return rc;
  for (int q = 0; q < h->Q && lags > 0; ++q) {
    if (metric_host)
      HIP_OK(hipMemcpyAsync(metric_host + (size_t)q * out_stride, h->rho + (size_t)q * nl + first, (size_t)lags * 4,
                            hipMemcpyDeviceToHost, h->stream));
    if (corr_host)
      HIP_OK(hipMemcpyAsync(static_cast<float2*>(corr_host) + (size_t)q * out_stride, h->r + (size_t)q * nl + first, (size_t)lags * 8,
                            hipMemcpyDeviceToHost, h->stream));
  }
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

int kcr_flush(kcr_corr* h) {
  if (!h) return fail("null correlator object");
  if (h->flushed) return fail("the stream was flushed; kcr_reset starts a new stream");
  if (h->lost) return fail("the stream state was lost when an earlier call failed after its first launch; kcr_reset starts a new stream");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  if (int rc = stream_call(h, nullptr, 0, nullptr, nullptr, 0, true)) return rc;
  h->flushed = true;
  return 0;
}

int kcr_blocks_dev(kcr_corr* h, const void* iq_dev, int64_t block_stride, int64_t nblocks, int64_t block_len, float* metric_dev,
                   void* corr_dev, int64_t out_stride) {
  if (!h) return fail("null correlator object");
  if (nblocks < 0) return fail("nblocks %lld must be >= 0", (long long)nblocks);
  if (block_stride < 0) return fail("block_stride %lld must be >= 0", (long long)block_stride);
  if (block_len < 0) return fail("block_len %lld must be >= 0", (long long)block_len);
  if (block_len < h->K) return fail("block_len %lld is shorter than the template of %d samples", (long long)block_len, h->K);
  if (block_len > h->max_in || nblocks > h->max_in / block_len)
    return fail("%lld blocks of %lld samples exceed max_in %lld", (long long)nblocks, (long long)block_len, h->max_in);
  if (nblocks > 0 && !iq_dev) return fail("null input pointer");
  if (int rc = check_iq_aligned(iq_dev, in_bytes(h))) return rc;
  const long long nl = block_len - h->K + 1;
  if ((metric_dev || corr_dev) && out_stride < nl)
    return fail("out_stride %lld is shorter than the %lld lags of a block", (long long)out_stride, nl);
  if (nblocks == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  ksa::corr::Args a = base_args(h);
  a.in = iq_dev;
  a.block_stride = block_stride;
  a.raw_len = (int)block_len;
  a.nl = (int)nl;
  a.metric_out = metric_dev;
  a.corr_out = static_cast<float2*>(corr_dev);
  a.out_stride = out_stride;
  if (int rc = launch_corr(h, a, nblocks)) return rc;
  return launch_pick(h, nblocks, (int)nl, 0, (int)nl, 0, false);
}

int kcr_set_params(kcr_corr* h, float threshold, float min_energy) {
  if (!h) return fail("null correlator object");
  if (int rc = check_params(threshold, min_energy)) return rc;
  h->threshold = threshold;                     // a launch carries its parameters by value: enqueued work keeps the old ones
  h->min_energy = min_energy;
  return 0;
}

int kcr_set_templates(kcr_corr* h, const float* templates_host) {
  if (!h) return fail("null correlator object");
  float ec[KCR_MAX_Q];
  if (int rc = check_templates(h->K, h->Q, templates_host, ec)) return rc;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  const std::vector<float> table = packed(h->K, h->Q, templates_host);
  HIP_OK(hipMemcpyAsync(h->tmpl, table.data(), table.size() * 4, hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipMemcpyAsync(h->ec, ec, (size_t)h->Q * 4, hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

int kcr_reset(kcr_corr* h) {
  if (!h) return fail("null correlator object");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  HIP_OK(hipMemsetAsync(h->events, 0, events_bytes(h), h->stream));
  HIP_OK(hipMemsetAsync(h->totals, 0, 16, h->stream));
  h->n_in = 0;
  h->decided = 0;
  h->lost = false;
  h->flushed = false;
  return 0;
}

int kcr_state(kcr_corr* h, int64_t* samples_in, int64_t* lags_done, int64_t* lags_decided) {
  if (!h) return fail("null correlator object");
  if (samples_in) *samples_in = h->n_in;
  if (lags_done) *lags_done = lags_after(h, h->n_in);
  if (lags_decided) *lags_decided = h->decided;
  return 0;
}

int kcr_read_events(kcr_corr* h, void* records_host, int64_t max_records, int64_t* stored, int64_t* total) {
  if (!h) return fail("null correlator object");
  if (max_records < 0) return fail("max_records %lld must be >= 0", (long long)max_records);
  if (!records_host && !stored && !total) return fail("null records, stored and total pointers");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  long long all = 0;
  HIP_OK(hipMemcpyAsync(&all, h->totals, 8, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  const long long kept = std::min<long long>(all, h->capacity);
  const long long n = records_host ? std::min<long long>(kept, max_records) : 0;
  if (n > 0) {
    HIP_OK(hipMemcpyAsync(records_host, h->events, (size_t)n * sizeof(kcr_event), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
  }
  if (stored) *stored = kept;
  if (total) *total = all;
  return 0;
}

int kcr_events_dev(kcr_corr* h, void** records_dev, int64_t** events_total_dev) {
  if (!h) return fail("null correlator object");
  if (!records_dev && !events_total_dev) return fail("null records and events_total out pointers");
  if (records_dev) *records_dev = h->events;
  if (events_total_dev) *events_total_dev = reinterpret_cast<int64_t*>(h->totals);
  return 0;
}

int kcr_clear_events(kcr_corr* h) {
  if (!h) return fail("null correlator object");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  HIP_OK(hipMemsetAsync(h->events, 0, events_bytes(h), h->stream));
  HIP_OK(hipMemsetAsync(h->totals, 0, 16, h->stream));
  return 0;
}

int kcr_kernel_info(kcr_corr* h, int32_t* threads, int32_t* lds_bytes, int32_t* vgprs, int32_t* grid, int32_t* tile_out) {
  if (!h) return fail("null correlator object");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  hipFuncAttributes attr;
  HIP_OK(hipFuncGetAttributes(&attr, h->kernel));
  if (threads) *threads = ksa::corr::THREADS;
  if (lds_bytes) *lds_bytes = (int32_t)attr.sharedSizeBytes + h->plan.lds_bytes;
  if (vgprs) *vgprs = attr.numRegs;
  if (grid) *grid = h->last_grid ? h->last_grid : h->cus * WG_PER_CU;
  if (tile_out) *tile_out = h->plan.tile_out;
  return 0;
}

}  // extern "C"
