// libksa_demod: host layer of include/ksa_demod.h (validation, launch planning, stream state, staging); kernels in
// kdm_kernels.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/ksa_demod.h"
#include "kdm_kernels.hpp"
#include "../csrc_shared/ksa_host.hpp"

namespace {

// A tile keeps (tile - 1) * D + T floats in LDS.  The largest of 1024 (four outputs per thread) and 256 outputs whose span stays
// within SPAN_FOUR lets four workgroups share a CU, which is what hides one workgroup's load phase behind the others' filter
// phase; else 256 outputs within SPAN_TWO (two workgroups per CU); 64 outputs always fit (63 * 256 + 4096 floats, 79 KiB).
constexpr int SPAN_FOUR = 9728;                 // + 2 * D of padding stays within 40 KiB
constexpr int SPAN_TWO = 19968;                 // + 2 * D of padding stays within 80 KiB

struct Plan {
  int per_thread = 1, tile_out = 0, pitch = 0, lds_bytes = 0;
};

Plan plan_for(int D, int T) {
  Plan p;
  p.tile_out = 255LL * D + T <= SPAN_TWO ? 256 : 64;
  if (1023LL * D + T <= SPAN_FOUR) p.tile_out = 1024;
  p.per_thread = p.tile_out == 1024 ? 4 : 1;
  const int span = (p.tile_out - 1) * D + T;
  p.pitch = (span + D - 1) / D;
  if (D > 1) p.pitch |= 1;                      // an odd pitch spreads the loader's consecutive samples over the banks
  p.lds_bytes = D * p.pitch * 4;
  return p;
}

const void* filter_kernel(int mode, int out_fmt, const Plan& p) {
  using namespace ksa::demod;
#define KDM_PICK(M)                                                                                                  \
  case M:                                                                                                            \
    if (out_fmt == KDM_OUT_S16)                                                                                      \
      return p.per_thread == 4 ? reinterpret_cast<const void*>(tile_kernel<M, 4, short>)                            \
                               : reinterpret_cast<const void*>(tile_kernel<M, 1, short>);                           \
    return p.per_thread == 4 ? reinterpret_cast<const void*>(tile_kernel<M, 4, float>)                              \
                             : reinterpret_cast<const void*>(tile_kernel<M, 1, float>);
  switch (mode) {
    KDM_PICK(MODE_AM)
    KDM_PICK(MODE_FM)
    default:
    KDM_PICK(MODE_PM)
  }
#undef KDM_PICK
}

const void* history_fn(int mode) {
  using namespace ksa::demod;
  switch (mode) {
    case MODE_AM: return reinterpret_cast<const void*>(history_kernel<MODE_AM>);
    case MODE_FM: return reinterpret_cast<const void*>(history_kernel<MODE_FM>);
    default: return reinterpret_cast<const void*>(history_kernel<MODE_PM>);
  }
}

}  // namespace

struct kdm_demod {
  int device = 0, mode = 0, out_fmt = 0, D = 1, T = 1, cus = 1, last_grid = 0, cur = 0;
  bool lost = false;                            // a stream call failed between its two launches: kdm_reset starts anew
  float pcm_scale = 32767.f;
  long long max_in = 0, out_cap = 0, n_in = 0, n_out = 0;
  Plan plan;
  const void* kernel = nullptr;
  float* taps = nullptr;                        // device [T]
  // device, the stream's state and the one being written: the last raw sample (two floats), then T - 1 demodulated samples
  float* state[2] = {nullptr, nullptr};
  void* out = nullptr;                          // device [out_cap] float32 or int16
  char* stage = nullptr;                        // kdm_process: the call's raw input
  long long stage_bytes = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_stream = nullptr;
};

namespace {

int out_bytes(const kdm_demod* h) { return h->out_fmt == KDM_OUT_S16 ? 2 : 4; }
size_t state_bytes(const kdm_demod* h) { return (size_t)(h->T - 1 + 2) * 4; }

void free_all(kdm_demod* h) {
  if (h->ev_stream) (void)hipEventDestroy(h->ev_stream);
  free_device({h->taps, h->state[0], h->state[1], h->out, h->stage});
  delete h;
}

ksa::demod::Args base_args(const kdm_demod* h) {
  ksa::demod::Args a{};
  a.taps = h->taps;
  a.D = h->D;
  a.T = h->T;
  a.magic = h->D > 1 ? (unsigned)((0xffffffffull / (unsigned)h->D) + 1) : 0u;
  a.pitch = h->plan.pitch;
  a.tile_out = h->plan.tile_out;
  a.pcm_scale = h->pcm_scale;
  return a;
}

int launch_filter(kdm_demod* h, ksa::demod::Args& a, long long nblocks) {
  a.tiles = (int)ceil_div(a.nout, h->plan.tile_out);
  const long long grid = (long long)a.tiles * nblocks;
  void* params[] = {&a};
  HIP_OK(hipLaunchKernel(h->kernel, dim3((unsigned)grid), dim3(ksa::demod::THREADS), params, (size_t)h->plan.lds_bytes, h->stream));
  h->last_grid = (int)grid;
  return 0;
}

// the next n samples of the stream at iq (device-visible), outputs to out (device, room checked by the caller)
int stream_call(kdm_demod* h, const void* iq, long long n, void* out, long long nout) {
  ksa::demod::Args a = base_args(h);
  a.iq = static_cast<const float2*>(iq);
  a.last = reinterpret_cast<const float2*>(h->state[h->cur]);
  a.hist = h->state[h->cur] + 2;
  a.out = out;
  a.raw_len = (int)n;
  a.hist_len = h->T - 1;
  a.off = (int)(ceil_div(h->n_in, h->D) * h->D - h->n_in);
  a.nout = (int)nout;
  if (nout > 0)
    if (int rc = launch_filter(h, a, 1)) return rc;
  if (h->T > 1 || h->mode == KDM_MODE_FM) {
    float* next = h->state[h->cur ^ 1];
    float* next_hist = next + 2;
    float2* next_last = reinterpret_cast<float2*>(next);
    void* params[] = {&a, &next_hist, &next_last};
    const unsigned grid = (unsigned)std::max(1LL, ceil_div(h->T - 1, ksa::demod::THREADS));
    const hipError_t e = hipLaunchKernel(history_fn(h->mode), dim3(grid), dim3(ksa::demod::THREADS), params, 0, h->stream);
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

int check_stream_args(kdm_demod* h, const void* iq, int64_t n_in, int64_t* nout) {
  if (!h) return fail("null demodulator object");
  if (n_in < 0) return fail("n_in %lld must be >= 0", (long long)n_in);
  if (n_in > h->max_in) return fail("n_in %lld exceeds max_in %lld", (long long)n_in, h->max_in);
  if (n_in > 0 && !iq) return fail("null input pointer");
  if (int rc = check_iq_aligned(iq, 8)) return rc;
  if (h->lost) return fail("the stream state was lost when an earlier call failed after its filter launch; kdm_reset starts a new stream");
  *nout = stream_outputs(h->n_in, n_in, h->D);
  return 0;
}

}  // namespace

extern "C" {

int kdm_abi_version(void) { return KDM_ABI_VERSION; }
const char* kdm_last_error(void) { return g_err.c_str(); }

int kdm_create(int32_t device, int32_t mode, int32_t decim, int32_t ntaps, const float* taps_host, int32_t out_fmt,
               float pcm_scale, int64_t max_in, kdm_demod** out) {
  if (!out) return fail("null out pointer");
  *out = nullptr;
  if (mode < KDM_MODE_AM || mode > KDM_MODE_PM) return fail("unknown mode %d", mode);
  if (out_fmt != KDM_OUT_F32 && out_fmt != KDM_OUT_S16) return fail("unknown output format %d", out_fmt);
  if (decim < 1 || decim > KDM_MAX_DECIM) return fail("decim %d outside 1..%d", decim, KDM_MAX_DECIM);
  if (ntaps < 1 || ntaps > KDM_MAX_TAPS) return fail("ntaps %d outside 1..%d", ntaps, KDM_MAX_TAPS);
  if (max_in < 1 || max_in > KDM_MAX_IN) return fail("max_in %lld outside 1..%d", (long long)max_in, KDM_MAX_IN);
  if (int rc = check_taps(ntaps, taps_host)) return rc;
  if (out_fmt == KDM_OUT_S16 && !(std::isfinite(pcm_scale) && pcm_scale > 0.f))
    return fail("pcm_scale %g must be finite and > 0", (double)pcm_scale);
  if (check_device(device)) return 1;

  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(device));
  kdm_demod* h = new kdm_demod;
  h->device = device; h->mode = mode; h->out_fmt = out_fmt; h->D = decim; h->T = ntaps; h->max_in = max_in;
  if (out_fmt == KDM_OUT_S16) h->pcm_scale = pcm_scale;
  h->out_cap = std::max(ceil_div(max_in, decim), (long long)(max_in / ntaps)) + 1;
  h->plan = plan_for(decim, ntaps);
  h->kernel = filter_kernel(mode, out_fmt, h->plan);
  int rc = 0;
  do {
    if ((rc = cu_count(device, &h->cus))) break;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->taps), (size_t)ntaps * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->state[0]), state_bytes(h));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->state[1]), state_bytes(h));
    if (e == hipSuccess) e = hipMalloc(&h->out, (size_t)h->out_cap * 4);
    if (e != hipSuccess) { rc = fail("hipMalloc of the demodulator's device memory failed: %s", hipGetErrorString(e)); break; }
    // the limit belongs to the kernel function, which objects of other D and T share: one value for every object of the process
    if (h->plan.lds_bytes > ksa::demod::LDS_MAX) { rc = fail("the plan's %d bytes of LDS exceed %d", h->plan.lds_bytes, ksa::demod::LDS_MAX); break; }
    e = hipFuncSetAttribute(h->kernel, hipFuncAttributeMaxDynamicSharedMemorySize, ksa::demod::LDS_MAX);
    if (e != hipSuccess) { rc = fail("the filter kernel cannot have %d bytes of LDS: %s", ksa::demod::LDS_MAX, hipGetErrorString(e)); break; }
    e = hipMemsetAsync(h->state[0], 0, state_bytes(h), h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h->taps, taps_host, (size_t)ntaps * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { rc = fail("filling the demodulator's device memory failed: %s", hipGetErrorString(e)); break; }
  } while (0);
  if (rc) {
    free_all(h);
    return rc;
  }
  *out = h;
  return 0;
}

void kdm_destroy(kdm_demod* h) {
  if (!h) return;
  DeviceGuard dev_guard;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  free_all(h);
}

int kdm_set_stream(kdm_demod* h, void* hip_stream) {
  if (!h) return fail("null demodulator object");
  return hand_over_stream(h->device, &h->stream, &h->ev_stream, hip_stream);
}

int kdm_synchronize(kdm_demod* h) {
  if (!h) return fail("null demodulator object");
  return synchronize_on(h->device, h->stream);
}

int kdm_out_count(kdm_demod* h, int64_t n_in, int64_t* n_out) {
  if (!h) return fail("null demodulator object");
  if (!n_out) return fail("null n_out pointer");
  if (n_in < 0) return fail("n_in %lld must be >= 0", (long long)n_in);
  *n_out = stream_outputs(h->n_in, n_in, h->D);
  return 0;
}

int kdm_process_dev(kdm_demod* h, const void* iq_dev, int64_t n_in, void* out_dev, int64_t out_capacity, int64_t* n_out) {
  int64_t nout = 0;
  if (int rc = check_stream_args(h, iq_dev, n_in, &nout)) return rc;
  if (out_dev && out_capacity < nout)
    return fail("output capacity %lld is too small for the call's %lld outputs", (long long)out_capacity, (long long)nout);
  if (n_out) *n_out = nout;
  if (n_in == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  return stream_call(h, iq_dev, n_in, out_dev ? out_dev : h->out, nout);
}

int kdm_process(kdm_demod* h, const void* iq_host, int64_t n_in, void* out_host, int64_t out_capacity, int64_t* n_out) {
  int64_t nout = 0;
  if (int rc = check_stream_args(h, iq_host, n_in, &nout)) return rc;
  if (nout > 0 && !out_host) return fail("null output pointer");
  if (out_capacity < nout)
    return fail("output capacity %lld is too small for the call's %lld outputs", (long long)out_capacity, (long long)nout);
  if (n_out) *n_out = nout;
  if (n_in == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  const long long bytes = (long long)n_in * 8;
  if (int rc = grow_device(&h->stage, &h->stage_bytes, bytes, h->stream)) return rc;
  HIP_OK(hipMemcpyAsync(h->stage, iq_host, (size_t)bytes, hipMemcpyHostToDevice, h->stream));
  if (int rc = stream_call(h, h->stage, n_in, h->out, nout)) return rc;
  if (nout > 0) HIP_OK(hipMemcpyAsync(out_host, h->out, (size_t)nout * out_bytes(h), hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

int kdm_blocks_dev(kdm_demod* h, const void* iq_dev, int64_t block_stride, int64_t nblocks, int64_t block_len, void* out_dev,
                   int64_t out_stride) {
  if (!h) return fail("null demodulator object");
  const int lead = h->mode == KDM_MODE_FM ? 1 : 0;
  if (nblocks < 0) return fail("nblocks %lld must be >= 0", (long long)nblocks);
  if (block_stride < 0) return fail("block_stride %lld must be >= 0", (long long)block_stride);
  if (block_len < h->T + lead)
    return fail("block_len %lld is shorter than the %d taps plus %d leading sample(s)", (long long)block_len, h->T, lead);
  if (block_len > h->max_in || nblocks > h->max_in / block_len)
    return fail("%lld blocks of %lld samples exceed max_in %lld", (long long)nblocks, (long long)block_len, h->max_in);
  if (nblocks > 0 && !iq_dev) return fail("null input pointer");
  if (int rc = check_iq_aligned(iq_dev, 8)) return rc;
  const long long M = (block_len - lead - h->T) / h->D + 1;
  if (out_dev && out_stride < M) return fail("out_stride %lld is shorter than the %lld outputs of a block", (long long)out_stride, M);
  if (!out_dev && nblocks * M > h->out_cap)
    return fail("output capacity %lld is too small for the call's %lld outputs", h->out_cap, nblocks * M);
  if (nblocks == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  ksa::demod::Args a = base_args(h);
  a.iq = static_cast<const float2*>(iq_dev);
  a.out = out_dev ? out_dev : h->out;
  a.block_stride = block_stride;
  a.out_stride = out_dev ? out_stride : M;
  a.raw_len = (int)block_len;
  a.off = lead;
  a.nout = (int)M;
  return launch_filter(h, a, nblocks);
}

int kdm_set_taps(kdm_demod* h, const float* taps_host) {
  if (!h) return fail("null demodulator object");
  if (int rc = check_taps(h->T, taps_host)) return rc;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  HIP_OK(hipMemcpyAsync(h->taps, taps_host, (size_t)h->T * 4, hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

int kdm_reset(kdm_demod* h) {
  if (!h) return fail("null demodulator object");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  HIP_OK(hipMemsetAsync(h->state[h->cur], 0, state_bytes(h), h->stream));
  h->n_in = h->n_out = 0;
  h->lost = false;
  return 0;
}

int kdm_state(kdm_demod* h, int64_t* samples_in, int64_t* samples_out) {
  if (!h) return fail("null demodulator object");
  if (samples_in) *samples_in = h->n_in;
  if (samples_out) *samples_out = h->n_out;
  return 0;
}

int kdm_out_dev(kdm_demod* h, void** out_dev, int64_t* capacity) {
  if (!h) return fail("null demodulator object");
  if (!out_dev) return fail("null out pointer");
  *out_dev = h->out;
  if (capacity) *capacity = h->out_cap;
  return 0;
}

int kdm_read_out(kdm_demod* h, void* out_host, int64_t first, int64_t count) {
  if (!h) return fail("null demodulator object");
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

int kdm_kernel_info(kdm_demod* h, int32_t* threads, int32_t* lds_bytes, int32_t* vgprs, int32_t* grid, int32_t* tile_out) {
  if (!h) return fail("null demodulator object");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  hipFuncAttributes attr;
  HIP_OK(hipFuncGetAttributes(&attr, h->kernel));
  if (threads) *threads = ksa::demod::THREADS;
  if (lds_bytes) *lds_bytes = (int32_t)attr.sharedSizeBytes + h->plan.lds_bytes;
  if (vgprs) *vgprs = attr.numRegs;
  if (grid) *grid = h->last_grid ? h->last_grid : h->cus * std::max(1, (160 * 1024) / std::max(1, h->plan.lds_bytes));
  if (tile_out) *tile_out = h->plan.tile_out;
  return 0;
}

}  // extern "C"
