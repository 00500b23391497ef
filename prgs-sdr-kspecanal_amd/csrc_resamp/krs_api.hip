// libksa_resamp: host layer of include/ksa_resamp.h (validation, launch planning, stream state, staging); kernels in
// krs_kernels.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>

#include "../../include/ksa_resamp.h"
#include "krs_kernels.hpp"
#include "../csrc_shared/ksa_host.hpp"

namespace {

constexpr long long GRID_MAX = 1LL << 20;       // workgroups per launch; a workgroup walks the tiles beyond

// A tile of W outputs keeps at most ((W - 1) M + L - 1) / L + P samples in LDS, one element of padding after every 32.
// W = 1024 (four outputs per thread) where that stays within 40 KiB, so that four workgroups share a CU; else W = 256, whose
// largest span (M = 16 L, P = 256, complex) is 35 KiB.
struct Plan {
  int per_thread = 1, tile_out = 0, lds_bytes = 0;
};

int span_bytes(int W, int L, int M, int P, int elem) {
  const long long span = ((long long)(W - 1) * M + L - 1) / L + P;
  return (int)((span + (span >> 5) + 1) * elem);
}

Plan plan_for(int type, int L, int M, int P) {
  const int elem = type == KRS_TYPE_C64 ? 8 : 4;
  Plan p;
  p.per_thread = span_bytes(1024, L, M, P, elem) <= ksa::resamp::LDS_FOUR ? 4 : 1;
  p.tile_out = 256 * p.per_thread;
  p.lds_bytes = span_bytes(p.tile_out, L, M, P, elem);
  return p;
}

const void* filter_kernel(int type, int out_fmt, const Plan& p) {
  using namespace ksa::resamp;
  if (type == KRS_TYPE_C64)
    return p.per_thread == 4 ? reinterpret_cast<const void*>(tile_kernel<float2, 4, float2>)
                             : reinterpret_cast<const void*>(tile_kernel<float2, 1, float2>);
  if (out_fmt == KRS_OUT_S16)
    return p.per_thread == 4 ? reinterpret_cast<const void*>(tile_kernel<float, 4, short>)
                             : reinterpret_cast<const void*>(tile_kernel<float, 1, short>);
  return p.per_thread == 4 ? reinterpret_cast<const void*>(tile_kernel<float, 4, float>)
                           : reinterpret_cast<const void*>(tile_kernel<float, 1, float>);
}

}  // namespace

struct krs_resamp {
  int device = 0, type = 0, out_fmt = 0, L = 1, M = 1, P = 1, cus = 1, last_grid = 0, cur = 0;
  bool lost = false;                            // a stream call failed between its two launches: krs_reset starts anew
  float pcm_scale = 32767.f;
  long long max_in = 0, out_cap = 0, n_in = 0, n_out = 0;
  Plan plan;
  const void* kernel = nullptr;
  float* taps = nullptr;                        // device g[P][L], the permuted table
  void* state[2] = {nullptr, nullptr};          // device, the stream's P - 1 history samples and the ones being written
  void* out = nullptr;                          // device [out_cap] values
  char* stage = nullptr;                        // krs_process: the call's input
  long long stage_bytes = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_stream = nullptr;
};

namespace {

int in_bytes(const krs_resamp* h) { return h->type == KRS_TYPE_C64 ? 8 : 4; }
int out_bytes(const krs_resamp* h) { return h->out_fmt == KRS_OUT_S16 ? 2 : in_bytes(h); }
size_t state_bytes(const krs_resamp* h) { return (size_t)std::max(1, h->P - 1) * in_bytes(h); }

// outputs of the stream once `seen` samples have arrived: ceil(seen L / M); seen <= 2^52 and L <= 2^10 keep it in int64
long long outputs_after(const krs_resamp* h, long long seen) { return ceil_div(seen * h->L, h->M); }

void free_all(krs_resamp* h) {
  if (h->ev_stream) (void)hipEventDestroy(h->ev_stream);
  free_device({h->taps, h->state[0], h->state[1], h->out, h->stage});
  delete h;
}

// g[q][i] = h[q L + (i M mod L)]: output m reads row q at m mod L
std::vector<float> permuted(const krs_resamp* h, const float* taps) {
  std::vector<float> g((size_t)h->L * h->P);
  for (int q = 0; q < h->P; ++q)
    for (int i = 0; i < h->L; ++i) g[(size_t)q * h->L + i] = taps[(size_t)q * h->L + (int)(((long long)i * h->M) % h->L)];
  return g;
}

ksa::resamp::Args base_args(const krs_resamp* h) {
  ksa::resamp::Args a{};
  a.taps = h->taps;
  a.L = h->L;
  a.M = h->M;
  a.P = h->P;
  a.tile_out = h->plan.tile_out;
  a.pcm_scale = h->pcm_scale;
  return a;
}

// output m_f is the first of the call: its position m_f M, relative to sample `origin` of the definition's x, as (n_f, p_f)
void set_first(const krs_resamp* h, ksa::resamp::Args& a, long long m_f, long long origin) {
  const long long t = m_f * h->M;               // <= 2^62 + M
  a.n_f = (int)(t / h->L - origin);
  a.p_f = (int)(t % h->L);
  a.c_f = m_f % h->L;
}

int launch_filter(krs_resamp* h, ksa::resamp::Args& a, long long nblocks) {
  a.tiles = ceil_div(a.nout, h->plan.tile_out);
  a.total = a.tiles * nblocks;
  const long long grid = std::min(a.total, GRID_MAX);
  void* params[] = {&a};
  HIP_OK(hipLaunchKernel(h->kernel, dim3((unsigned)grid), dim3(ksa::resamp::THREADS), params, (size_t)h->plan.lds_bytes, h->stream));
  h->last_grid = (int)grid;
  return 0;
}

// the next n samples of the stream at in (device-visible), outputs to out (device, room checked by the caller)
int stream_call(krs_resamp* h, const void* in, long long n, void* out, long long nout) {
  ksa::resamp::Args a = base_args(h);
  a.in = in;
  a.hist = h->state[h->cur];
  a.out = out;
  a.raw_len = (int)n;
  a.hist_len = h->P - 1;
  a.nout = nout;
  // virtual sample v is sample n_in - (P - 1) + v of the stream: output m's oldest sample n(m) - (P - 1) is virtual n(m) - n_in
  set_first(h, a, h->n_out, h->n_in);
  if (nout > 0)
    if (int rc = launch_filter(h, a, 1)) return rc;
  if (h->P > 1) {
    void* next = h->state[h->cur ^ 1];
    void* params[] = {&a, &next};
    const void* fn = h->type == KRS_TYPE_C64 ? reinterpret_cast<const void*>(ksa::resamp::history_kernel<float2>)
                                             : reinterpret_cast<const void*>(ksa::resamp::history_kernel<float>);
    const unsigned grid = (unsigned)ceil_div(h->P - 1, ksa::resamp::THREADS);
    const hipError_t e = hipLaunchKernel(fn, dim3(grid), dim3(ksa::resamp::THREADS), params, 0, h->stream);
    if (e != hipSuccess) {                        // outputs may be written, history and counts are not: the stream is lost
      h->lost = nout > 0;
      return fail("launching the history kernel failed: %s", hipGetErrorString(e));
    }
    h->cur ^= 1;
  }
  h->n_in += n;
  h->n_out += nout;
  return 0;
}

int check_stream_args(krs_resamp* h, const void* in, int64_t n_in, int64_t* nout) {
  if (!h) return fail("null resampler object");
  if (n_in < 0) return fail("n_in %lld must be >= 0", (long long)n_in);
  if (n_in > h->max_in) return fail("n_in %lld exceeds max_in %lld", (long long)n_in, h->max_in);
  if (n_in > 0 && !in) return fail("null input pointer");
  if (int rc = check_iq_aligned(in, in_bytes(h))) return rc;
  if (h->lost) return fail("the stream state was lost when an earlier call failed after its filter launch; krs_reset starts a new stream");
  if (n_in > KRS_MAX_POSITION - h->n_in)
    return fail("n_in %lld would take the stream from %lld samples past 2^52", (long long)n_in, h->n_in);
  *nout = outputs_after(h, h->n_in + n_in) - h->n_out;
  return 0;
}

int check_create(int32_t type, int32_t L, int32_t M, int32_t P, const float* taps_host, int32_t out_fmt, float pcm_scale) {
  if (type != KRS_TYPE_F32 && type != KRS_TYPE_C64) return fail("unknown sample type %d", type);
  if (out_fmt != KRS_OUT_SAME && out_fmt != KRS_OUT_S16) return fail("unknown output format %d", out_fmt);
  if (L < 1 || L > KRS_MAX_L) return fail("L %d outside 1..%d", L, KRS_MAX_L);
  if (M < 1 || M > KRS_MAX_M) return fail("M %d outside 1..%d", M, KRS_MAX_M);
  if (M > KRS_MAX_RATIO * L) return fail("M %d exceeds %d L = %d: decimate by an integer in front", M, KRS_MAX_RATIO, KRS_MAX_RATIO * L);
  const int g = std::gcd(L, M);
  if (g != 1) return fail("L / M = %d / %d is not reduced, use %d / %d", L, M, L / g, M / g);
  if (P < 1 || P > KRS_MAX_PHASE_TAPS) return fail("taps_per_phase %d outside 1..%d", P, KRS_MAX_PHASE_TAPS);
  if ((long long)L * P > KRS_MAX_TAPS) return fail("L x taps_per_phase = %lld taps exceed %d", (long long)L * P, KRS_MAX_TAPS);
  if (out_fmt == KRS_OUT_S16 && type == KRS_TYPE_C64) return fail("int16 output wants real input, the sample type is complex64");
  if (int rc = check_taps(L * P, taps_host)) return rc;
  if (out_fmt == KRS_OUT_S16 && !(std::isfinite(pcm_scale) && pcm_scale > 0.f))
    return fail("pcm_scale %g must be finite and > 0", (double)pcm_scale);
  return 0;
}

}  // namespace

extern "C" {

int krs_abi_version(void) { return KRS_ABI_VERSION; }
const char* krs_last_error(void) { return g_err.c_str(); }

int krs_create(int32_t device, int32_t type, int32_t L, int32_t M, int32_t taps_per_phase, const float* taps_host,
               int32_t out_fmt, float pcm_scale, int64_t max_in, krs_resamp** out) {
  if (!out) return fail("null out pointer");
  *out = nullptr;
  const int P = taps_per_phase;
  if (max_in < 1 || max_in > KRS_MAX_IN) return fail("max_in %lld outside 1..%d", (long long)max_in, KRS_MAX_IN);
  if (int rc = check_create(type, L, M, P, taps_host, out_fmt, pcm_scale)) return rc;
  if (check_device(device)) return 1;

  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(device));
  krs_resamp* h = new krs_resamp;
  h->device = device; h->type = type; h->out_fmt = out_fmt; h->L = L; h->M = M; h->P = P; h->max_in = max_in;
  if (out_fmt == KRS_OUT_S16) h->pcm_scale = pcm_scale;
  h->out_cap = ceil_div(max_in * L, M) + 1;
  h->plan = plan_for(type, L, M, P);
  h->kernel = filter_kernel(type, out_fmt, h->plan);
  const std::vector<float> g = permuted(h, taps_host);
  int rc = 0;
  do {
    if ((rc = cu_count(device, &h->cus))) break;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->taps), g.size() * 4);
    if (e == hipSuccess) e = hipMalloc(&h->state[0], state_bytes(h));
    if (e == hipSuccess) e = hipMalloc(&h->state[1], state_bytes(h));
    if (e == hipSuccess) e = hipMalloc(&h->out, (size_t)h->out_cap * out_bytes(h));
    if (e != hipSuccess) { rc = fail("hipMalloc of the resampler's device memory failed: %s", hipGetErrorString(e)); break; }
    e = hipMemsetAsync(h->state[0], 0, state_bytes(h), h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h->taps, g.data(), g.size() * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { rc = fail("filling the resampler's device memory failed: %s", hipGetErrorString(e)); break; }
  } while (0);
  if (rc) {
    free_all(h);
    return rc;
  }
  *out = h;
  return 0;
}

void krs_destroy(krs_resamp* h) {
  if (!h) return;
  DeviceGuard dev_guard;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  free_all(h);
}

int krs_set_stream(krs_resamp* h, void* hip_stream) {
  if (!h) return fail("null resampler object");
  return hand_over_stream(h->device, &h->stream, &h->ev_stream, hip_stream);
}

int krs_synchronize(krs_resamp* h) {
  if (!h) return fail("null resampler object");
  return synchronize_on(h->device, h->stream);
}

int krs_out_count(krs_resamp* h, int64_t n_in, int64_t* n_out) {
  if (!h) return fail("null resampler object");
  if (!n_out) return fail("null n_out pointer");
  if (n_in < 0) return fail("n_in %lld must be >= 0", (long long)n_in);
  if (n_in > KRS_MAX_POSITION - h->n_in)
    return fail("n_in %lld would take the stream from %lld samples past 2^52", (long long)n_in, h->n_in);
  *n_out = outputs_after(h, h->n_in + n_in) - h->n_out;
  return 0;
}

int krs_process_dev(krs_resamp* h, const void* in_dev, int64_t n_in, void* out_dev, int64_t out_capacity, int64_t* n_out) {
  int64_t nout = 0;
  if (int rc = check_stream_args(h, in_dev, n_in, &nout)) return rc;
  if ((out_dev ? out_capacity : h->out_cap) < nout)
    return fail("output capacity %lld is too small for the call's %lld outputs", (long long)(out_dev ? out_capacity : h->out_cap),
                (long long)nout);
  if (n_out) *n_out = nout;
  if (n_in == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  return stream_call(h, in_dev, n_in, out_dev ? out_dev : h->out, nout);
}

int krs_process(krs_resamp* h, const void* in_host, int64_t n_in, void* out_host, int64_t out_capacity, int64_t* n_out) {
  int64_t nout = 0;
  if (int rc = check_stream_args(h, in_host, n_in, &nout)) return rc;
  if (nout > 0 && !out_host) return fail("null output pointer");
  if (out_capacity < nout || h->out_cap < nout)
    return fail("output capacity %lld is too small for the call's %lld outputs", (long long)std::min<long long>(out_capacity, h->out_cap),
                (long long)nout);
  if (n_out) *n_out = nout;
  if (n_in == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  const long long bytes = (long long)n_in * in_bytes(h);
  if (int rc = grow_device(&h->stage, &h->stage_bytes, bytes, h->stream)) return rc;
  HIP_OK(hipMemcpyAsync(h->stage, in_host, (size_t)bytes, hipMemcpyHostToDevice, h->stream));
  if (int rc = stream_call(h, h->stage, n_in, h->out, nout)) return rc;
  if (nout > 0) HIP_OK(hipMemcpyAsync(out_host, h->out, (size_t)nout * out_bytes(h), hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

int krs_blocks_dev(krs_resamp* h, const void* in_dev, int64_t block_stride, int64_t nblocks, int64_t block_len, void* out_dev,
                   int64_t out_stride) {
  if (!h) return fail("null resampler object");
  if (nblocks < 0) return fail("nblocks %lld must be >= 0", (long long)nblocks);
  if (block_stride < 0) return fail("block_stride %lld must be >= 0", (long long)block_stride);
  if (block_len < 0) return fail("block_len %lld must be >= 0", (long long)block_len);
  if (block_len > h->max_in || (block_len > 0 && nblocks > h->max_in / block_len))
    return fail("%lld blocks of %lld samples exceed max_in %lld", (long long)nblocks, (long long)block_len, h->max_in);
  const long long first = ceil_div((long long)(h->P - 1) * h->L, h->M);
  const long long J = ceil_div(block_len * h->L, h->M) - first;
  if (J < 1)
    return fail("block_len %lld yields no output past the start-up transient of %d taps per phase", (long long)block_len, h->P);
  if (nblocks > 0 && !in_dev) return fail("null input pointer");
  if (int rc = check_iq_aligned(in_dev, in_bytes(h))) return rc;
  if (out_dev && out_stride < J) return fail("out_stride %lld is shorter than the %lld outputs of a block", (long long)out_stride, J);
  if (!out_dev && nblocks * J > h->out_cap)
    return fail("output capacity %lld is too small for the call's %lld outputs", h->out_cap, nblocks * J);
  if (nblocks == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  ksa::resamp::Args a = base_args(h);
  a.in = in_dev;
  a.out = out_dev ? out_dev : h->out;
  a.block_stride = block_stride;
  a.out_stride = out_dev ? out_stride : J;
  a.raw_len = (int)block_len;
  a.nout = J;
  set_first(h, a, first, h->P - 1);             // virtual sample v is sample v of the block: the oldest of output m is n(m) - (P - 1)
  return launch_filter(h, a, nblocks);
}

int krs_set_taps(krs_resamp* h, const float* taps_host) {
  if (!h) return fail("null resampler object");
  if (int rc = check_taps(h->L * h->P, taps_host)) return rc;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  const std::vector<float> g = permuted(h, taps_host);
  HIP_OK(hipMemcpyAsync(h->taps, g.data(), g.size() * 4, hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

int krs_reset_at(krs_resamp* h, int64_t samples_in) {
  if (!h) return fail("null resampler object");
  if (samples_in < 0 || samples_in > KRS_MAX_POSITION) return fail("samples_in %lld outside 0..2^52", (long long)samples_in);
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  HIP_OK(hipMemsetAsync(h->state[h->cur], 0, state_bytes(h), h->stream));
  h->n_in = samples_in;
  h->n_out = outputs_after(h, samples_in);
  h->lost = false;
  return 0;
}

int krs_reset(krs_resamp* h) { return krs_reset_at(h, 0); }

int krs_state(krs_resamp* h, int64_t* samples_in, int64_t* samples_out) {
  if (!h) return fail("null resampler object");
  if (samples_in) *samples_in = h->n_in;
  if (samples_out) *samples_out = h->n_out;
  return 0;
}

int krs_out_dev(krs_resamp* h, void** out_dev, int64_t* capacity) {
  if (!h) return fail("null resampler object");
  if (!out_dev) return fail("null out pointer");
  *out_dev = h->out;
  if (capacity) *capacity = h->out_cap;
  return 0;
}

int krs_read_out(krs_resamp* h, void* out_host, int64_t first, int64_t count) {
  if (!h) return fail("null resampler object");
  if (first < 0) return fail("first %lld must be >= 0", (long long)first);
  if (count < 0) return fail("count %lld must be >= 0", (long long)count);
  if (first > h->out_cap || count > h->out_cap - first)
    return fail("values %lld .. %lld lie outside the output buffer of %lld", (long long)first, (long long)(first + count), h->out_cap);
  if (count > 0 && !out_host) return fail("null output pointer");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  if (count > 0)
    HIP_OK(hipMemcpyAsync(out_host, static_cast<const char*>(h->out) + (size_t)first * out_bytes(h), (size_t)count * out_bytes(h),
                          hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

int krs_kernel_info(krs_resamp* h, int32_t* threads, int32_t* lds_bytes, int32_t* vgprs, int32_t* grid, int32_t* tile_out) {
  if (!h) return fail("null resampler object");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  hipFuncAttributes attr;
  HIP_OK(hipFuncGetAttributes(&attr, h->kernel));
  if (threads) *threads = ksa::resamp::THREADS;
  if (lds_bytes) *lds_bytes = (int32_t)attr.sharedSizeBytes + h->plan.lds_bytes;
  if (vgprs) *vgprs = attr.numRegs;
  if (grid) *grid = h->last_grid ? h->last_grid : h->cus * std::max(1, (160 * 1024) / std::max(1, h->plan.lds_bytes));
  if (tile_out) *tile_out = h->plan.tile_out;
  return 0;
}

}  // extern "C"
