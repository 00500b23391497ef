// libksa_ddc: host layer of include/ksa_ddc.h (validation, launch planning, stream state, staging); kernels in kdc_kernels.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/ksa_ddc.h"
#include "kdc_kernels.hpp"
#include "../csrc_shared/ksa_host.hpp"

static_assert(KDC_FMT_C64 == ksa::iq::FMT_C64 && KDC_FMT_U8 == ksa::iq::FMT_U8 && KDC_FMT_S8 == ksa::iq::FMT_S8 &&
              KDC_FMT_S16 == ksa::iq::FMT_S16, "the formats of the header are the kernels' and iq_sample_bytes's");

namespace {

// The tile form keeps (tile - 1) * D + T samples in LDS.  Up to SPAN_SMALL two workgroups share a CU and a thread takes as many
// outputs (4, 2, 1) as fit; up to SPAN_LARGE one workgroup of one output per thread has the CU alone; beyond, the reduce form.
constexpr int SPAN_SMALL = 7680;
constexpr int SPAN_LARGE = 17408;               // + 2 * D of padding stays below 160 KiB

struct Plan {
  int form = KDC_FORM_TILE, per_thread = 1, threads = 0, tile_out = 0, pitch = 0, lds_bytes = 0;
};

Plan plan_for(int D, int T) {
  using namespace ksa::ddc;
  Plan p;
  int r = 0;
  for (int cand : {4, 2, 1})
    if (!r && (long long)(TILE_THREADS * cand - 1) * D + T <= SPAN_SMALL) r = cand;
  if (!r && (long long)(TILE_THREADS - 1) * D + T <= SPAN_LARGE) r = 1;
  if (r) {
    p.form = KDC_FORM_TILE;
    p.per_thread = r;
    p.threads = TILE_THREADS;
    p.tile_out = TILE_THREADS * r;
    const int span = (p.tile_out - 1) * D + T;
    p.pitch = (span + D - 1) / D;
    if (D > 1) p.pitch |= 1;                    // an odd pitch spreads the loader's consecutive samples over the banks
    p.lds_bytes = D * p.pitch * 8;
  } else {
    p.form = KDC_FORM_REDUCE;
    p.threads = RED_THREADS;
    p.tile_out = RED_OUT;
    p.lds_bytes = (RED_CHUNK + RED_WAVES * RED_OUT) * 8 + ((T + 3) & ~3) * 4;
  }
  return p;
}

const void* filter_kernel(int fmt, const Plan& p) {
  using namespace ksa::ddc;
#define KDC_PICK(F)                                                                              \
  case F:                                                                                        \
    if (p.form == KDC_FORM_REDUCE) return reinterpret_cast<const void*>(reduce_kernel<F>);       \
    if (p.per_thread == 4) return reinterpret_cast<const void*>(tile_kernel<F, 4>);              \
    if (p.per_thread == 2) return reinterpret_cast<const void*>(tile_kernel<F, 2>);              \
    return reinterpret_cast<const void*>(tile_kernel<F, 1>);
  switch (fmt) {
    KDC_PICK(FMT_C64)
    KDC_PICK(FMT_U8)
    KDC_PICK(FMT_S8)
    default:
    KDC_PICK(FMT_S16)
  }
#undef KDC_PICK
}

const void* history_fn(int fmt) {
  using namespace ksa::ddc;
  switch (fmt) {
    case FMT_C64: return reinterpret_cast<const void*>(history_kernel<FMT_C64>);
    case FMT_U8: return reinterpret_cast<const void*>(history_kernel<FMT_U8>);
    case FMT_S8: return reinterpret_cast<const void*>(history_kernel<FMT_S8>);
    default: return reinterpret_cast<const void*>(history_kernel<FMT_S16>);
  }
}

}  // namespace

struct kdc_ddc {
  int device = 0, fmt = 0, D = 1, T = 1, cus = 1, last_grid = 0, cur_hist = 0;
  float u8_offset = 127.5f, u8_inv_scale = 1.f / 127.5f;
  long long max_in = 0, out_cap = 0, n_in = 0, n_out = 0;
  unsigned long long phase = 0, phase_inc = 0;
  Plan plan;
  const void* kernel = nullptr;
  float* taps = nullptr;                        // device [T]
  float2* hist[2] = {nullptr, nullptr};         // device [max(T - 1, 1)] each: the history and the one being written
  float2* out = nullptr;                        // device [out_cap]
  char* stage = nullptr;                        // kdc_process: the call's raw input
  long long stage_bytes = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_stream = nullptr;
};

namespace {

void free_all(kdc_ddc* h) {
  if (h->ev_stream) (void)hipEventDestroy(h->ev_stream);
  free_device({h->taps, h->hist[0], h->hist[1], h->out, h->stage});
  delete h;
}

ksa::ddc::Args base_args(const kdc_ddc* h) {
  ksa::ddc::Args a{};
  a.taps = h->taps;
  a.D = h->D;
  a.T = h->T;
  a.magic = h->D > 1 ? (unsigned)((0xffffffffull / (unsigned)h->D) + 1) : 0u;
  a.pitch = h->plan.pitch;
  a.tile_out = h->plan.tile_out;
  a.u8_offset = h->u8_offset;
  a.u8_inv_scale = h->u8_inv_scale;
  a.phase_inc = h->phase_inc;
  return a;
}

int launch_filter(kdc_ddc* h, ksa::ddc::Args& a, long long nblocks) {
  a.tiles = (int)ceil_div(a.nout, h->plan.tile_out);
  const long long grid = (long long)a.tiles * nblocks;
  void* params[] = {&a};
  HIP_OK(hipLaunchKernel(h->kernel, dim3((unsigned)grid), dim3(h->plan.threads), params, (size_t)h->plan.lds_bytes, h->stream));
  h->last_grid = (int)grid;
  return 0;
}

// the next n samples of the stream at iq (device-visible), outputs to out (device, room checked by the caller)
int stream_call(kdc_ddc* h, const void* iq, long long n, float2* out, long long nout) {
  ksa::ddc::Args a = base_args(h);
  a.iq = iq;
  a.hist = h->hist[h->cur_hist];
  a.out = out;
  a.phase0 = h->phase;
  a.raw_len = (int)n;
  a.hist_len = h->T - 1;
  a.off = (int)(ceil_div(h->n_in, h->D) * h->D - h->n_in);
  a.nout = (int)nout;
  if (nout > 0)
    if (int rc = launch_filter(h, a, 1)) return rc;
  if (h->T > 1) {
    float2* next = h->hist[h->cur_hist ^ 1];
    void* params[] = {&a, &next};
    HIP_OK(hipLaunchKernel(history_fn(h->fmt), dim3((unsigned)ceil_div(h->T - 1, 256)), dim3(256), params, 0, h->stream));
    h->cur_hist ^= 1;
  }
  h->phase += (unsigned long long)n * h->phase_inc;
  h->n_in += n;
  h->n_out += nout;
  return 0;
}

int check_stream_args(kdc_ddc* h, const void* iq, int64_t n_in, int64_t* nout) {
  if (!h) return fail("null down-converter object");
  if (n_in < 0) return fail("n_in %lld must be >= 0", (long long)n_in);
  if (n_in > h->max_in) return fail("n_in %lld exceeds max_in %lld", (long long)n_in, h->max_in);
  if (n_in > 0 && !iq) return fail("null input pointer");
  if (int rc = check_iq_aligned(iq, iq_sample_bytes(h->fmt))) return rc;
  *nout = stream_outputs(h->n_in, n_in, h->D);
  return 0;
}

}  // namespace

extern "C" {

int kdc_abi_version(void) { return KDC_ABI_VERSION; }
const char* kdc_last_error(void) { return g_err.c_str(); }

int kdc_create(int32_t device, int32_t fmt, float u8_offset, float u8_scale, int32_t decim, int32_t ntaps,
               const float* taps_host, uint64_t phase_inc, int64_t max_in, kdc_ddc** out) {
  if (!out) return fail("null out pointer");
  *out = nullptr;
  if (check_iq_format(fmt)) return 1;
  if (decim < 1 || decim > KDC_MAX_DECIM) return fail("decim %d outside 1..%d", decim, KDC_MAX_DECIM);
  if (ntaps < 1 || ntaps > KDC_MAX_TAPS) return fail("ntaps %d outside 1..%d", ntaps, KDC_MAX_TAPS);
  if (max_in < 1 || max_in > KDC_MAX_IN) return fail("max_in %lld outside 1..%d", (long long)max_in, KDC_MAX_IN);
  if (int rc = check_taps(ntaps, taps_host)) return rc;
  if (check_u8_scaling(fmt, u8_offset, u8_scale)) return 1;
  if (check_device(device)) return 1;

  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(device));
  kdc_ddc* h = new kdc_ddc;
  h->device = device; h->fmt = fmt; h->D = decim; h->T = ntaps; h->max_in = max_in; h->phase_inc = phase_inc;
  if (fmt == KDC_FMT_U8) { h->u8_offset = u8_offset; h->u8_inv_scale = 1.0f / u8_scale; }
  h->out_cap = std::max(ceil_div(max_in, decim), (long long)(max_in / ntaps)) + 1;
  h->plan = plan_for(decim, ntaps);
  h->kernel = filter_kernel(fmt, h->plan);
  int rc = 0;
  do {
    if ((rc = cu_count(device, &h->cus))) break;
    const size_t hist_bytes = (size_t)std::max(ntaps - 1, 1) * 8;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->taps), (size_t)ntaps * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->hist[0]), hist_bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->hist[1]), hist_bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->out), (size_t)h->out_cap * 8);
    if (e != hipSuccess) { rc = fail("hipMalloc of the down-converter's device memory failed: %s", hipGetErrorString(e)); break; }
    e = hipFuncSetAttribute(h->kernel, hipFuncAttributeMaxDynamicSharedMemorySize, h->plan.lds_bytes);
    if (e != hipSuccess) { rc = fail("the filter kernel cannot have %d bytes of LDS: %s", h->plan.lds_bytes, hipGetErrorString(e)); break; }
    e = hipMemsetAsync(h->hist[0], 0, hist_bytes, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h->taps, taps_host, (size_t)ntaps * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { rc = fail("filling the down-converter's device memory failed: %s", hipGetErrorString(e)); break; }
  } while (0);
  if (rc) {
    free_all(h);
    return rc;
  }
  *out = h;
  return 0;
}

void kdc_destroy(kdc_ddc* h) {
  if (!h) return;
  DeviceGuard dev_guard;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  free_all(h);
}

int kdc_set_stream(kdc_ddc* h, void* hip_stream) {
  if (!h) return fail("null down-converter object");
  return hand_over_stream(h->device, &h->stream, &h->ev_stream, hip_stream);
}

int kdc_synchronize(kdc_ddc* h) {
  if (!h) return fail("null down-converter object");
  return synchronize_on(h->device, h->stream);
}

int kdc_out_count(kdc_ddc* h, int64_t n_in, int64_t* n_out) {
  if (!h) return fail("null down-converter object");
  if (!n_out) return fail("null n_out pointer");
  if (n_in < 0) return fail("n_in %lld must be >= 0", (long long)n_in);
  *n_out = stream_outputs(h->n_in, n_in, h->D);
  return 0;
}

int kdc_process_dev(kdc_ddc* h, const void* iq_dev, int64_t n_in, void* out_dev, int64_t out_capacity, int64_t* n_out) {
  int64_t nout = 0;
  if (int rc = check_stream_args(h, iq_dev, n_in, &nout)) return rc;
  if (out_dev && out_capacity < nout)
    return fail("output capacity %lld is too small for the call's %lld outputs", (long long)out_capacity, (long long)nout);
  if (n_out) *n_out = nout;
  if (n_in == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  return stream_call(h, iq_dev, n_in, out_dev ? static_cast<float2*>(out_dev) : h->out, nout);
}

int kdc_process(kdc_ddc* h, const void* iq_host, int64_t n_in, void* out_host, int64_t out_capacity, int64_t* n_out) {
  int64_t nout = 0;
  if (int rc = check_stream_args(h, iq_host, n_in, &nout)) return rc;
  if (nout > 0 && !out_host) return fail("null output pointer");
  if (out_capacity < nout)
    return fail("output capacity %lld is too small for the call's %lld outputs", (long long)out_capacity, (long long)nout);
  if (n_out) *n_out = nout;
  if (n_in == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  const long long bytes = (long long)n_in * iq_sample_bytes(h->fmt);
  if (int rc = grow_device(&h->stage, &h->stage_bytes, bytes, h->stream)) return rc;
  HIP_OK(hipMemcpyAsync(h->stage, iq_host, (size_t)bytes, hipMemcpyHostToDevice, h->stream));
  if (int rc = stream_call(h, h->stage, n_in, h->out, nout)) return rc;
  if (nout > 0) HIP_OK(hipMemcpyAsync(out_host, h->out, (size_t)nout * 8, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

int kdc_blocks_dev(kdc_ddc* h, const void* iq_dev, int64_t block_stride, int64_t nblocks, int64_t block_len, void* out_dev,
                   int64_t out_stride) {
  if (!h) return fail("null down-converter object");
  if (nblocks < 0) return fail("nblocks %lld must be >= 0", (long long)nblocks);
  if (block_stride < 0) return fail("block_stride %lld must be >= 0", (long long)block_stride);
  if (block_len < h->T) return fail("block_len %lld is shorter than the %d taps", (long long)block_len, h->T);
  if (block_len > h->max_in || nblocks > h->max_in / block_len)
    return fail("%lld blocks of %lld samples exceed max_in %lld", (long long)nblocks, (long long)block_len, h->max_in);
  if (nblocks > 0 && !iq_dev) return fail("null input pointer");
  if (int rc = check_iq_aligned(iq_dev, iq_sample_bytes(h->fmt))) return rc;
  const long long M = (block_len - h->T) / h->D + 1;
  if (out_dev && out_stride < M) return fail("out_stride %lld is shorter than the %lld outputs of a block", (long long)out_stride, M);
  if (!out_dev && nblocks * M > h->out_cap)
    return fail("output capacity %lld is too small for the call's %lld outputs", h->out_cap, nblocks * M);
  if (nblocks == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  ksa::ddc::Args a = base_args(h);
  a.iq = iq_dev;
  a.out = out_dev ? static_cast<float2*>(out_dev) : h->out;
  a.block_stride = block_stride;
  a.out_stride = out_dev ? out_stride : M;
  a.phase0 = 0;
  a.raw_len = (int)block_len;
  a.nout = (int)M;
  return launch_filter(h, a, nblocks);
}

int kdc_set_tuning(kdc_ddc* h, uint64_t phase_inc) {
  if (!h) return fail("null down-converter object");
  h->phase_inc = phase_inc;
  return 0;
}

int kdc_set_taps(kdc_ddc* h, const float* taps_host) {
  if (!h) return fail("null down-converter object");
  if (int rc = check_taps(h->T, taps_host)) return rc;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  HIP_OK(hipMemcpyAsync(h->taps, taps_host, (size_t)h->T * 4, hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

int kdc_reset(kdc_ddc* h) {
  if (!h) return fail("null down-converter object");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  HIP_OK(hipMemsetAsync(h->hist[h->cur_hist], 0, (size_t)std::max(h->T - 1, 1) * 8, h->stream));
  h->phase = 0;
  h->n_in = h->n_out = 0;
  return 0;
}

int kdc_state(kdc_ddc* h, int64_t* samples_in, int64_t* samples_out, uint64_t* phase) {
  if (!h) return fail("null down-converter object");
  if (samples_in) *samples_in = h->n_in;
  if (samples_out) *samples_out = h->n_out;
  if (phase) *phase = h->phase;
  return 0;
}

int kdc_out_dev(kdc_ddc* h, void** out_dev, int64_t* capacity) {
  if (!h) return fail("null down-converter object");
  if (!out_dev) return fail("null out pointer");
  *out_dev = h->out;
  if (capacity) *capacity = h->out_cap;
  return 0;
}

int kdc_kernel_info(kdc_ddc* h, int32_t* threads, int32_t* lds_bytes, int32_t* vgprs, int32_t* grid, int32_t* tile_out,
                    int32_t* form) {
  if (!h) return fail("null down-converter object");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  hipFuncAttributes attr;
  HIP_OK(hipFuncGetAttributes(&attr, h->kernel));
  if (threads) *threads = h->plan.threads;
  if (lds_bytes) *lds_bytes = (int32_t)attr.sharedSizeBytes + h->plan.lds_bytes;
  if (vgprs) *vgprs = attr.numRegs;
  if (grid) *grid = h->last_grid ? h->last_grid : h->cus * std::max(1, (160 * 1024) / std::max(1, h->plan.lds_bytes));
  if (tile_out) *tile_out = h->plan.tile_out;
  if (form) *form = h->plan.form;
  return 0;
}

}  // extern "C"
