// libksa_chan: host layer of include/ksa_chan.h (validation, launch planning, stream state, staging); kernels in kch_kernels.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/ksa_chan.h"
#include "kch_kernels.hpp"
#include "../csrc_shared/ksa_host.hpp"

static_assert(KCH_FMT_C64 == ksa::iq::FMT_C64 && KCH_FMT_U8 == ksa::iq::FMT_U8 && KCH_FMT_S8 == ksa::iq::FMT_S8 &&
              KCH_FMT_S16 == ksa::iq::FMT_S16, "the formats of the header are the kernels' and iq_sample_bytes's");

namespace {

constexpr int LDS_TWO = 80 * 1024, LDS_ONE = 160 * 1024;   // two workgroups per CU, or one
constexpr int WORK_VALUES = 8192;                          // W * M at most: 64 KiB of workspace
constexpr int MAX_W = 256;

struct Plan {
  int W = 1, logW = 0, pitch = 0, lds_bytes = 0, threads = 256;
};

int lds_for(int M, int D, int T, int W) {
  const int pitch = W > 1 ? M + 1 : M;
  return 8 * (std::max(M / 2, 2) + ((W * pitch + 1) & ~1) + (W - 1) * D + T);
}

// The largest power of two W <= min(256, 8192 / M) whose LDS stays at 80 KiB, if that is 16 columns or all that M allows;
// else the largest that stays at 160 KiB.  Threads: 256 where four workgroups share a CU's LDS (40 KiB), 512 where two do, 1024
// where one has it alone: 16 waves per CU either way.  A function of (M, O, P) alone.
Plan plan_for(int M, int O, int P) {
  const int D = M / O, T = M * P, wmax = std::min(MAX_W, WORK_VALUES / M);
  int W = 0;
  for (int c = wmax; c >= 1 && !W; c >>= 1)
    if (lds_for(M, D, T, c) <= LDS_TWO && c >= std::min(16, wmax)) W = c;
  for (int c = wmax; c >= 1 && !W; c >>= 1)
    if (lds_for(M, D, T, c) <= LDS_ONE) W = c;
  Plan p;
  p.W = W;
  while ((1 << p.logW) < W) ++p.logW;
  p.pitch = W > 1 ? M + 1 : M;
  p.lds_bytes = lds_for(M, D, T, W);
  p.threads = std::max(M, p.lds_bytes <= LDS_TWO / 2 ? 256 : p.lds_bytes <= LDS_TWO ? 512 : 1024);   // never below M: the kernel relies on it
  return p;
}

const void* main_kernel(int fmt) {
  using namespace ksa::chan;
  switch (fmt) {
    case FMT_C64: return reinterpret_cast<const void*>(chan_kernel<FMT_C64>);
    case FMT_U8: return reinterpret_cast<const void*>(chan_kernel<FMT_U8>);
    case FMT_S8: return reinterpret_cast<const void*>(chan_kernel<FMT_S8>);
    default: return reinterpret_cast<const void*>(chan_kernel<FMT_S16>);
  }
}

const void* history_fn(int fmt) {
  using namespace ksa::chan;
  switch (fmt) {
    case FMT_C64: return reinterpret_cast<const void*>(history_kernel<FMT_C64>);
    case FMT_U8: return reinterpret_cast<const void*>(history_kernel<FMT_U8>);
    case FMT_S8: return reinterpret_cast<const void*>(history_kernel<FMT_S8>);
    default: return reinterpret_cast<const void*>(history_kernel<FMT_S16>);
  }
}

}  // namespace

struct kch_chan {
  int device = 0, fmt = 0, M = 2, logM = 1, O = 1, P = 1, D = 2, T = 2, cus = 1, last_grid = 0, cur_hist = 0;
  float u8_offset = 127.5f, u8_inv_scale = 1.f / 127.5f;
  long long max_in = 0, own_stride = 0, out_cap = 0, n_in = 0, n_out = 0;
  long long rows = 0, row_stride = 0;           // what the last call left in the own buffer
  bool lost = false;                            // a stream call failed between its two launches: kch_reset starts anew
  Plan plan;
  const void* kernel = nullptr;
  float* taps = nullptr;                        // device [T]
  float2* tw = nullptr;                         // device [max(M / 2, 1)]
  float2* hist[2] = {nullptr, nullptr};         // device [T - 1] each: the history and the one being written
  float2* out = nullptr;                        // device [out_cap]
  double* power = nullptr;                      // device [M]
  char* stage = nullptr;                        // kch_process: the call's raw input
  long long stage_bytes = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_stream = nullptr;
};

namespace {

void free_all(kch_chan* h) {
  if (h->ev_stream) (void)hipEventDestroy(h->ev_stream);
  free_device({h->taps, h->tw, h->hist[0], h->hist[1], h->out, h->power, h->stage});
  delete h;
}

ksa::chan::Args base_args(const kch_chan* h) {
  ksa::chan::Args a{};
  a.taps = h->taps;
  a.tw = h->tw;
  a.W = h->plan.W;
  a.logW = h->plan.logW;
  a.M = h->M;
  a.logM = h->logM;
  a.D = h->D;
  a.T = h->T;
  a.P = h->P;
  a.rot = 4 / h->O;
  a.pitch = h->plan.pitch;
  a.u8_offset = h->u8_offset;
  a.u8_inv_scale = h->u8_inv_scale;
  return a;
}

hipError_t launch_main(kch_chan* h, ksa::chan::Args& a, long long nblocks) {
  a.tiles = (int)ceil_div(a.ncol, h->plan.W);
  const long long grid = (long long)a.tiles * nblocks;
  void* params[] = {&a};
  const hipError_t e = hipLaunchKernel(h->kernel, dim3((unsigned)grid), dim3((unsigned)h->plan.threads), params, (size_t)h->plan.lds_bytes, h->stream);
  if (e == hipSuccess) h->last_grid = (int)grid;
  return e;
}

// the next n samples of the stream at iq (device-visible), ncol columns to out at chan_stride (room checked by the caller)
int stream_call(kch_chan* h, const void* iq, long long n, float2* out, long long chan_stride, long long ncol) {
  ksa::chan::Args a = base_args(h);
  a.iq = iq;
  a.hist = h->hist[h->cur_hist];
  a.out = out;
  a.chan_stride = chan_stride;
  a.raw_len = (int)n;
  a.hist_len = h->T - 1;
  a.off = (int)(ceil_div(h->n_in, h->D) * h->D - h->n_in);
  a.ncol = (int)ncol;
  a.m_first = (int)(h->n_out & 3);
  if (ncol > 0) {
    const hipError_t e = launch_main(h, a, 1);
    if (e != hipSuccess) return fail("launching the channelizer kernel failed: %s", hipGetErrorString(e));
  }
  float2* next = h->hist[h->cur_hist ^ 1];
  void* params[] = {&a, &next};
  const hipError_t e = hipLaunchKernel(history_fn(h->fmt), dim3((unsigned)ceil_div(h->T - 1, 256)), dim3(256), params, 0, h->stream);
  if (e != hipSuccess) {
    if (ncol > 0) h->lost = true;
    return fail("launching the history kernel failed: %s", hipGetErrorString(e));
  }
  h->cur_hist ^= 1;
  h->n_in += n;
  h->n_out += ncol;
  return 0;
}

int check_stream_args(kch_chan* h, const void* iq, int64_t n_in, int64_t* ncol) {
  if (!h) return fail("null channelizer object");
  if (n_in < 0) return fail("n_in %lld must be >= 0", (long long)n_in);
  if (n_in > h->max_in) return fail("n_in %lld exceeds max_in %lld", (long long)n_in, h->max_in);
  if (n_in > 0 && !iq) return fail("null input pointer");
  if (int rc = check_iq_aligned(iq, iq_sample_bytes(h->fmt))) return rc;
  if (h->lost) return fail("the stream state was lost when an earlier call failed after its filter launch; kch_reset starts a new stream");
  *ncol = stream_outputs(h->n_in, n_in, h->D);
  return 0;
}

}  // namespace

extern "C" {

int kch_abi_version(void) { return KCH_ABI_VERSION; }
const char* kch_last_error(void) { return g_err.c_str(); }

int kch_create(int32_t device, int32_t fmt, float u8_offset, float u8_scale, int32_t nchan, int32_t oversample,
               int32_t taps_per_branch, const float* taps_host, int64_t max_in, kch_chan** out) {
  if (!out) return fail("null out pointer");
  *out = nullptr;
  if (check_iq_format(fmt)) return 1;
  if (nchan < KCH_MIN_CHAN || nchan > KCH_MAX_CHAN || (nchan & (nchan - 1)))
    return fail("nchan %d must be a power of two, %d..%d", nchan, KCH_MIN_CHAN, KCH_MAX_CHAN);
  if (oversample != 1 && oversample != 2 && oversample != 4) return fail("oversample %d must be 1, 2 or 4", oversample);
  if (nchan / oversample < 1) return fail("the decimation nchan / oversample = %d / %d is below 1", nchan, oversample);
  if (taps_per_branch < 1 || taps_per_branch > KCH_MAX_BRANCH_TAPS)
    return fail("taps_per_branch %d outside 1..%d", taps_per_branch, KCH_MAX_BRANCH_TAPS);
  if ((long long)nchan * taps_per_branch > KCH_MAX_TAPS)
    return fail("the prototype of nchan * taps_per_branch = %d taps exceeds %d", nchan * taps_per_branch, KCH_MAX_TAPS);
  if (max_in < 1 || max_in > KCH_MAX_IN) return fail("max_in %lld outside 1..%d", (long long)max_in, KCH_MAX_IN);
  const int T = nchan * taps_per_branch;
  if (int rc = check_taps(T, taps_host)) return rc;
  if (check_u8_scaling(fmt, u8_offset, u8_scale)) return 1;
  if (check_device(device)) return 1;

  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(device));
  kch_chan* h = new kch_chan;
  h->device = device; h->fmt = fmt; h->M = nchan; h->O = oversample; h->P = taps_per_branch;
  h->D = nchan / oversample; h->T = T; h->max_in = max_in;
  h->logM = 0;
  while ((1 << h->logM) < nchan) ++h->logM;
  if (fmt == KCH_FMT_U8) { h->u8_offset = u8_offset; h->u8_inv_scale = 1.0f / u8_scale; }
  h->own_stride = ceil_div(max_in, h->D) + 1;
  h->out_cap = h->own_stride * nchan;
  h->rows = nchan;
  h->row_stride = h->own_stride;
  h->plan = plan_for(nchan, oversample, taps_per_branch);
  h->kernel = main_kernel(fmt);
  // exp(+2 pi i k / M) in float64, rounded once; exact on the axes
  const int ntw = std::max(nchan / 2, 1);
  std::vector<float2> tw((size_t)ntw);
  for (int k = 0; k < ntw; ++k) {
    const double ang = 2.0 * 3.14159265358979323846 * (double)k / (double)nchan;
    tw[(size_t)k] = make_float2((float)std::cos(ang), (float)std::sin(ang));
  }
  tw[0] = make_float2(1.f, 0.f);
  if (nchan >= 4) tw[(size_t)(nchan / 4)] = make_float2(0.f, 1.f);
  int rc = 0;
  do {
    if ((rc = cu_count(device, &h->cus))) break;
    const size_t hist_bytes = (size_t)(T - 1) * 8;            // T >= 2
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->taps), (size_t)T * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->tw), (size_t)ntw * 8);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->hist[0]), hist_bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->hist[1]), hist_bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->power), (size_t)nchan * 8);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->out), (size_t)h->out_cap * 8);
    if (e != hipSuccess) { rc = fail("hipMalloc of the channelizer's device memory failed: %s", hipGetErrorString(e)); break; }
    // the limit belongs to the kernel function, which objects of every (M, O, P) of one format share: one value for every object of
    // the process, the most any plan may ask for
    if (h->plan.lds_bytes > LDS_ONE) { rc = fail("the plan's %d bytes of LDS exceed %d", h->plan.lds_bytes, LDS_ONE); break; }
    e = hipFuncSetAttribute(h->kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_ONE);
    if (e != hipSuccess) { rc = fail("the channelizer kernel cannot have %d bytes of LDS: %s", LDS_ONE, hipGetErrorString(e)); break; }
    e = hipMemsetAsync(h->hist[0], 0, hist_bytes, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h->taps, taps_host, (size_t)T * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h->tw, tw.data(), (size_t)ntw * 8, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { rc = fail("filling the channelizer's device memory failed: %s", hipGetErrorString(e)); break; }
  } while (0);
  if (rc) {
    free_all(h);
    return rc;
  }
  *out = h;
  return 0;
}

void kch_destroy(kch_chan* h) {
  if (!h) return;
  DeviceGuard dev_guard;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  free_all(h);
}

int kch_set_stream(kch_chan* h, void* hip_stream) {
  if (!h) return fail("null channelizer object");
  return hand_over_stream(h->device, &h->stream, &h->ev_stream, hip_stream);
}

int kch_synchronize(kch_chan* h) {
  if (!h) return fail("null channelizer object");
  return synchronize_on(h->device, h->stream);
}

int kch_out_count(kch_chan* h, int64_t n_in, int64_t* n_out) {
  if (!h) return fail("null channelizer object");
  if (!n_out) return fail("null n_out pointer");
  if (n_in < 0) return fail("n_in %lld must be >= 0", (long long)n_in);
  *n_out = stream_outputs(h->n_in, n_in, h->D);
  return 0;
}

int kch_process_dev(kch_chan* h, const void* iq_dev, int64_t n_in, void* out_dev, int64_t chan_stride, int64_t* n_out) {
  int64_t ncol = 0;
  if (int rc = check_stream_args(h, iq_dev, n_in, &ncol)) return rc;
  if (out_dev && chan_stride < 0) return fail("chan_stride %lld must be >= 0", (long long)chan_stride);
  if (out_dev && chan_stride < ncol)
    return fail("chan_stride %lld is shorter than the call's %lld columns", (long long)chan_stride, (long long)ncol);
  if (n_in == 0) {
    if (n_out) *n_out = 0;
    return 0;
  }
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  if (int rc = stream_call(h, iq_dev, n_in, out_dev ? static_cast<float2*>(out_dev) : h->out, out_dev ? chan_stride : h->own_stride, ncol))
    return rc;
  if (!out_dev) { h->rows = h->M; h->row_stride = h->own_stride; }
  if (n_out) *n_out = ncol;                       // only a call that went through reports columns
  return 0;
}

int kch_process(kch_chan* h, const void* iq_host, int64_t n_in, void* out_host, int64_t chan_stride, int64_t* n_out) {
  int64_t ncol = 0;
  if (int rc = check_stream_args(h, iq_host, n_in, &ncol)) return rc;
  if (ncol > 0 && !out_host) return fail("null output pointer");
  if (chan_stride < 0) return fail("chan_stride %lld must be >= 0", (long long)chan_stride);
  if (chan_stride < ncol)
    return fail("chan_stride %lld is shorter than the call's %lld columns", (long long)chan_stride, (long long)ncol);
  if (n_in == 0) {
    if (n_out) *n_out = 0;
    return 0;
  }
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  const long long bytes = (long long)n_in * iq_sample_bytes(h->fmt);
  if (int rc = grow_device(&h->stage, &h->stage_bytes, bytes, h->stream)) return rc;
  HIP_OK(hipMemcpyAsync(h->stage, iq_host, (size_t)bytes, hipMemcpyHostToDevice, h->stream));
  if (int rc = stream_call(h, h->stage, n_in, h->out, h->own_stride, ncol)) return rc;
  h->rows = h->M;
  h->row_stride = h->own_stride;
  if (ncol > 0)
    HIP_OK(hipMemcpy2DAsync(out_host, (size_t)chan_stride * 8, h->out, (size_t)h->own_stride * 8, (size_t)ncol * 8, (size_t)h->M,
                            hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  if (n_out) *n_out = ncol;                       // only a call that went through reports columns
  return 0;
}

int kch_blocks_dev(kch_chan* h, const void* iq_dev, int64_t block_stride, int64_t nblocks, int64_t block_len, void* out_dev,
                   int64_t chan_stride) {
  if (!h) return fail("null channelizer object");
  if (nblocks < 0) return fail("nblocks %lld must be >= 0", (long long)nblocks);
  if (block_stride < 0) return fail("block_stride %lld must be >= 0", (long long)block_stride);
  const long long first = ceil_div(h->T - 1, h->D);
  if (block_len < first * h->D + 1)
    return fail("block_len %lld is shorter than the %lld samples of the first full column", (long long)block_len, first * h->D + 1);
  if (block_len > h->max_in || nblocks > h->max_in / block_len)
    return fail("%lld blocks of %lld samples exceed max_in %lld", (long long)nblocks, (long long)block_len, h->max_in);
  if (nblocks > 0 && !iq_dev) return fail("null input pointer");
  if (int rc = check_iq_aligned(iq_dev, iq_sample_bytes(h->fmt))) return rc;
  const long long J = (block_len - 1) / h->D - first + 1;
  if (out_dev && chan_stride < J)
    return fail("chan_stride %lld is shorter than the %lld columns of a block", (long long)chan_stride, J);
  if (nblocks == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  ksa::chan::Args a = base_args(h);
  a.iq = iq_dev;
  a.out = out_dev ? static_cast<float2*>(out_dev) : h->out;
  a.block_stride = block_stride;
  a.chan_stride = out_dev ? chan_stride : J;
  a.raw_len = (int)block_len;
  a.hist_len = 0;
  a.off = (int)(first * h->D - (h->T - 1));
  a.ncol = (int)J;
  a.m_first = (int)(first & 3);
  const hipError_t e = launch_main(h, a, nblocks);
  if (e != hipSuccess) return fail("launching the channelizer kernel failed: %s", hipGetErrorString(e));
  if (!out_dev) { h->rows = nblocks * h->M; h->row_stride = J; }
  return 0;
}

int kch_channel_power(kch_chan* h, int64_t first, int64_t count, double* power_host) {
  if (!h) return fail("null channelizer object");
  if (!power_host) return fail("null power pointer");
  if (first < 0 || count < 0 || first > h->row_stride || count > h->row_stride - first)
    return fail("values %lld .. %lld + %lld lie outside the %lld values of a row", (long long)first, (long long)first, (long long)count,
                h->row_stride);
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  const float2* buf = h->out;
  long long stride = h->row_stride, f = first;
  int M = h->M, nrows = (int)(h->rows / h->M), cnt = (int)count;
  double* power = h->power;
  void* params[] = {&buf, &stride, &M, &nrows, &f, &cnt, &power};
  HIP_OK(hipLaunchKernel(reinterpret_cast<const void*>(ksa::chan::power_kernel), dim3((unsigned)h->M), dim3(256), params, 256 * sizeof(double),
                         h->stream));
  HIP_OK(hipMemcpyAsync(power_host, h->power, (size_t)h->M * 8, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

int kch_set_taps(kch_chan* h, const float* taps_host) {
  if (!h) return fail("null channelizer object");
  if (int rc = check_taps(h->T, taps_host)) return rc;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  HIP_OK(hipMemcpyAsync(h->taps, taps_host, (size_t)h->T * 4, hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

int kch_reset(kch_chan* h) {
  if (!h) return fail("null channelizer object");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  HIP_OK(hipMemsetAsync(h->hist[h->cur_hist], 0, (size_t)(h->T - 1) * 8, h->stream));
  h->n_in = h->n_out = 0;
  h->lost = false;
  return 0;
}

int kch_state(kch_chan* h, int64_t* samples_in, int64_t* samples_out) {
  if (!h) return fail("null channelizer object");
  if (samples_in) *samples_in = h->n_in;
  if (samples_out) *samples_out = h->n_out;
  return 0;
}

int kch_out_dev(kch_chan* h, void** out_dev, int64_t* rows, int64_t* row_stride, int64_t* capacity) {
  if (!h) return fail("null channelizer object");
  if (!out_dev) return fail("null out pointer");
  *out_dev = h->out;
  if (rows) *rows = h->rows;
  if (row_stride) *row_stride = h->row_stride;
  if (capacity) *capacity = h->out_cap;
  return 0;
}

int kch_read_out(kch_chan* h, void* out_host, int64_t chan, int64_t first, int64_t count) {
  if (!h) return fail("null channelizer object");
  if (chan < 0 || chan >= h->rows) return fail("row %lld outside 0..%lld", (long long)chan, h->rows - 1);
  if (first < 0 || count < 0 || first > h->row_stride || count > h->row_stride - first)
    return fail("values %lld .. %lld + %lld lie outside the %lld values of a row", (long long)first, (long long)first, (long long)count,
                h->row_stride);
  if (count > 0 && !out_host) return fail("null output pointer");
  if (count == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  HIP_OK(hipMemcpyAsync(out_host, h->out + chan * h->row_stride + first, (size_t)count * 8, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

int kch_kernel_info(kch_chan* h, int32_t* threads, int32_t* lds_bytes, int32_t* vgprs, int32_t* grid, int32_t* tile_cols,
                    int32_t* form) {
  if (!h) return fail("null channelizer object");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  hipFuncAttributes attr;
  HIP_OK(hipFuncGetAttributes(&attr, h->kernel));
  if (threads) *threads = h->plan.threads;
  if (lds_bytes) *lds_bytes = (int32_t)attr.sharedSizeBytes + h->plan.lds_bytes;
  if (vgprs) *vgprs = attr.numRegs;
  if (grid) *grid = h->last_grid ? h->last_grid : h->cus * std::max(1, LDS_ONE / std::max(1, h->plan.lds_bytes));
  if (tile_cols) *tile_cols = h->plan.W;
  if (form) *form = KCH_FORM_LDS;
  return 0;
}

}  // extern "C"
