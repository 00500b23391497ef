// libksa_iqfix: host layer of include/ksa_iqfix.h (validation, launch planning, the solve, staging); kernels in
// kqf_kernels.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/ksa_iqfix.h"
#include "kqf_kernels.hpp"
#include "../csrc_shared/ksa_host.hpp"

static_assert(sizeof(kqf_coeffs) == 32, "kqf_coeffs has no padding");
static_assert(KQF_FMT_C64 == ksa::iq::FMT_C64 && KQF_FMT_U8 == ksa::iq::FMT_U8 && KQF_FMT_S8 == ksa::iq::FMT_S8 &&
                  KQF_FMT_S16 == ksa::iq::FMT_S16,
              "the formats of the header are the kernels'");

struct kqf_corrector {
  int device = 0, fmt = 0, last_grid = 0;
  bool last_apply = true, last_acc = false;     // the kernel of the last launch
  float u8_offset = 127.5f, u8_inv_scale = 1.f / 127.5f;
  kqf_coeffs co = {0.f, 0.f, 0.f, 1.f, 0, 0, 0};
  long long max_in = 0;
  long long count = 0;                          // the host's copy of sums[5]
  long long* sums = nullptr;                    // device [6]
  long long* partials = nullptr;                // device [MAX_GRID][NSUMS]
  float2* out = nullptr;                        // device [max_in], made when first needed
  char* stage = nullptr;                        // kqf_apply: the call's input
  long long stage_bytes = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_stream = nullptr;
};

namespace {

using ksa::iqfix::MAX_GRID;
using ksa::iqfix::NSUMS;
using ksa::iqfix::THREADS;
using ksa::iqfix::TILE;

int in_bytes(const kqf_corrector* h) { return iq_sample_bytes(h->fmt); }

void free_all(kqf_corrector* h) {
  if (h->ev_stream) (void)hipEventDestroy(h->ev_stream);
  free_device({h->sums, h->partials, h->out, h->stage});
  delete h;
}

// the library's own output buffer; the caller has set the device
int ensure_out(kqf_corrector* h) {
  if (h->out) return 0;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->out), (size_t)h->max_in * sizeof(float2));
  if (e != hipSuccess) {
    h->out = nullptr;
    return fail("hipMalloc of the corrector's output buffer of %lld samples failed: %s", h->max_in, hipGetErrorString(e));
  }
  return 0;
}

template <int FMT> const void* kernel_of(bool apply, bool acc) {
  using namespace ksa::iqfix;
  return apply ? (acc ? reinterpret_cast<const void*>(fix_kernel<FMT, true, true>) : reinterpret_cast<const void*>(fix_kernel<FMT, true, false>))
               : reinterpret_cast<const void*>(fix_kernel<FMT, false, true>);
}

const void* kernel_of(int fmt, bool apply, bool acc) {
  switch (fmt) {
    case KQF_FMT_C64: return kernel_of<KQF_FMT_C64>(apply, acc);
    case KQF_FMT_U8: return kernel_of<KQF_FMT_U8>(apply, acc);
    case KQF_FMT_S8: return kernel_of<KQF_FMT_S8>(apply, acc);
    default: return kernel_of<KQF_FMT_S16>(apply, acc);
  }
}

template <int FMT> void launch_fmt(kqf_corrector* h, const ksa::iqfix::Args& a, int grid, bool apply, bool acc) {
  using namespace ksa::iqfix;
  const dim3 g((unsigned)grid), wg(THREADS);
  if (apply && acc) hipLaunchKernelGGL((fix_kernel<FMT, true, true>), g, wg, 0, h->stream, a);
  else if (apply) hipLaunchKernelGGL((fix_kernel<FMT, true, false>), g, wg, 0, h->stream, a);
  else hipLaunchKernelGGL((fix_kernel<FMT, false, true>), g, wg, 0, h->stream, a);
}

// the argument checks of both block forms; *total = the samples of the call
int check_blocks(kqf_corrector* h, const void* iq_dev, int64_t block_stride, int64_t nblocks, int64_t block_len, bool acc, long long* total) {
  if (!h) return fail("null corrector object");
  if (nblocks < 0) return fail("nblocks %lld must be >= 0", (long long)nblocks);
  if (block_stride < 0) return fail("block_stride %lld must be >= 0", (long long)block_stride);
  if (block_len < 0) return fail("block_len %lld must be >= 0", (long long)block_len);
  if (block_len > h->max_in || (block_len > 0 && nblocks > h->max_in / block_len))
    return fail("%lld blocks of %lld samples exceed max_in %lld", (long long)nblocks, (long long)block_len, h->max_in);
  if (nblocks > 0 && block_len > 0 && !iq_dev) return fail("null input pointer");
  if (int rc = check_iq_aligned(iq_dev, in_bytes(h))) return rc;
  *total = (long long)nblocks * (long long)block_len;
  if (acc && *total > KQF_MAX_COUNT - h->count)
    return fail("%lld samples would take the count of the sums from %lld past 2^30; kqf_clear_stats starts them anew", *total, h->count);
  return 0;
}

// nblocks blocks of block_len > 0 samples at `in`; out may be null without apply.  The caller has set the device.
int run(kqf_corrector* h, const void* in, long long block_stride, long long nblocks, long long block_len, float2* out,
        long long out_stride, bool apply, bool acc) {
  ksa::iqfix::Args a{};
  a.in = in;
  a.out = out;
  a.partials = h->partials;
  a.block_stride = block_stride;
  a.out_stride = out_stride;
  a.tiles = (int)ceil_div(block_len, TILE);
  a.ntiles = a.tiles * nblocks;
  a.u8_offset = h->u8_offset;
  a.u8_inv_scale = h->u8_inv_scale;
  a.dc_i = h->co.dc_i;
  a.dc_q = h->co.dc_q;
  a.c = h->co.c;
  a.d = h->co.d;
  a.len = (int)block_len;
  const int grid = (int)std::min<long long>(a.ntiles, MAX_GRID);
  switch (h->fmt) {
    case KQF_FMT_C64: launch_fmt<KQF_FMT_C64>(h, a, grid, apply, acc); break;
    case KQF_FMT_U8: launch_fmt<KQF_FMT_U8>(h, a, grid, apply, acc); break;
    case KQF_FMT_S8: launch_fmt<KQF_FMT_S8>(h, a, grid, apply, acc); break;
    default: launch_fmt<KQF_FMT_S16>(h, a, grid, apply, acc); break;
  }
  HIP_OK(hipGetLastError());
  h->last_grid = grid;
  h->last_apply = apply;
  h->last_acc = acc;
  if (acc) {
    const long long total = nblocks * block_len;
    hipLaunchKernelGGL(ksa::iqfix::finish_kernel, dim3(1), dim3(THREADS), 0, h->stream, h->partials, grid, total, h->sums);
    HIP_OK(hipGetLastError());
    h->count += total;
  }
  return 0;
}

// Sums -> coefficients in float64, every operation rounded on its own.
kqf_coeffs solve_sums(const long long s[6], int mode) {
#pragma clang fp contract(off)
  kqf_coeffs r = {0.f, 0.f, 0.f, 1.f, 0, mode, s[5]};
  if (s[5] == 0) {
    r.flags = KQF_FLAG_EMPTY;
    return r;
  }
  const double u = (double)s[5] * 1073741824.0;
  const double mI = (double)s[0] / u, mQ = (double)s[1] / u;
  const double vII = (double)s[2] / u - mI * mI;
  const double vQQ = (double)s[3] / u - mQ * mQ;
  const double vIQ = (double)s[4] / u - mI * mQ;
  if (mode & KQF_MODE_DC) {
    r.dc_i = (float)mI;
    r.dc_q = (float)mQ;
  }
  if (mode & KQF_MODE_IQ) {
    bool valid = false;
    if (vII > 0.0) {
      const double q = vIQ / vII;
      const double w = vQQ - q * vIQ;
      if (w > 0.0) {
        const double ratio = vII / w;
        if (ratio >= 0.00390625 && ratio <= 256.0) {
          const double d = std::sqrt(ratio);
          const double c = -(d * q);
          r.c = (float)c;
          r.d = (float)d;
          valid = true;
        }
      }
    }
    if (!valid) r.flags |= KQF_FLAG_DEGENERATE;
  }
  return r;
}

}  // namespace

extern "C" {

int kqf_abi_version(void) { return KQF_ABI_VERSION; }
const char* kqf_last_error(void) { return g_err.c_str(); }

int kqf_create(int32_t device, int32_t fmt, float u8_offset, float u8_scale, int64_t max_in, kqf_corrector** out) {
  if (!out) return fail("null out pointer");
  *out = nullptr;
  if (check_iq_format(fmt)) return 1;
  if (max_in < 1 || max_in > KQF_MAX_IN) return fail("max_in %lld outside 1..%d", (long long)max_in, KQF_MAX_IN);
  if (check_u8_scaling(fmt, u8_offset, u8_scale)) return 1;
  if (check_device(device)) return 1;

  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(device));
  kqf_corrector* h = new kqf_corrector;
  h->device = device; h->fmt = fmt; h->max_in = max_in;
  if (fmt == KQF_FMT_U8) { h->u8_offset = u8_offset; h->u8_inv_scale = 1.0f / u8_scale; }
  int rc = 0;
  do {
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->sums), 6 * sizeof(long long));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->partials), (size_t)MAX_GRID * NSUMS * sizeof(long long));
    if (e != hipSuccess) { rc = fail("hipMalloc of the corrector's device memory failed: %s", hipGetErrorString(e)); break; }
    e = hipMemsetAsync(h->sums, 0, 6 * sizeof(long long), h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { rc = fail("filling the corrector's device memory failed: %s", hipGetErrorString(e)); break; }
  } while (0);
  if (rc) {
    free_all(h);
    return rc;
  }
  *out = h;
  return 0;
}

void kqf_destroy(kqf_corrector* h) {
  if (!h) return;
  DeviceGuard dev_guard;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  free_all(h);
}

int kqf_set_stream(kqf_corrector* h, void* hip_stream) {
  if (!h) return fail("null corrector object");
  return hand_over_stream(h->device, &h->stream, &h->ev_stream, hip_stream);
}

int kqf_synchronize(kqf_corrector* h) {
  if (!h) return fail("null corrector object");
  return synchronize_on(h->device, h->stream);
}

int kqf_blocks_dev(kqf_corrector* h, const void* iq_dev, int64_t block_stride, int64_t nblocks, int64_t block_len, void* out_dev,
                   int64_t out_stride, int32_t accumulate) {
  long long total = 0;
  if (int rc = check_blocks(h, iq_dev, block_stride, nblocks, block_len, accumulate != 0, &total)) return rc;
  if (out_dev && out_stride < block_len)
    return fail("out_stride %lld is shorter than the %lld samples of a block", (long long)out_stride, (long long)block_len);
  if (out_dev && reinterpret_cast<uintptr_t>(out_dev) % 8) return fail("output pointer is not aligned to the 8 bytes of a complex64");
  if (total == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  if (!out_dev) {
    if (int rc = ensure_out(h)) return rc;
  }
  return run(h, iq_dev, block_stride, nblocks, block_len, out_dev ? static_cast<float2*>(out_dev) : h->out,
             out_dev ? (long long)out_stride : (long long)block_len, true, accumulate != 0);
}

int kqf_accumulate_dev(kqf_corrector* h, const void* iq_dev, int64_t block_stride, int64_t nblocks, int64_t block_len) {
  long long total = 0;
  if (int rc = check_blocks(h, iq_dev, block_stride, nblocks, block_len, true, &total)) return rc;
  if (total == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  return run(h, iq_dev, block_stride, nblocks, block_len, nullptr, 0, false, true);
}

int kqf_apply(kqf_corrector* h, const void* iq_host, int64_t n, void* out_host, int32_t accumulate) {
  if (!h) return fail("null corrector object");
  if (n < 0) return fail("n %lld must be >= 0", (long long)n);
  if (n > h->max_in) return fail("n %lld exceeds max_in %lld", (long long)n, h->max_in);
  if (n > 0 && !iq_host) return fail("null input pointer");
  if (n > 0 && !out_host && !accumulate) return fail("null output pointer");
  if (accumulate && n > KQF_MAX_COUNT - h->count)
    return fail("%lld samples would take the count of the sums from %lld past 2^30; kqf_clear_stats starts them anew", (long long)n, h->count);
  if (n == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  const long long bytes = (long long)n * in_bytes(h);
  if (int rc = grow_device(&h->stage, &h->stage_bytes, bytes, h->stream)) return rc;
  if (out_host) {
    if (int rc = ensure_out(h)) return rc;
  }
  HIP_OK(hipMemcpyAsync(h->stage, iq_host, (size_t)bytes, hipMemcpyHostToDevice, h->stream));
  if (int rc = run(h, h->stage, n, 1, n, h->out, n, out_host != nullptr, accumulate != 0)) return rc;
  if (out_host) HIP_OK(hipMemcpyAsync(out_host, h->out, (size_t)n * sizeof(float2), hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

int kqf_solve(kqf_corrector* h, int32_t mode, kqf_coeffs* out) {
  if (!h) return fail("null corrector object");
  if (mode <= 0 || (mode & ~(KQF_MODE_DC | KQF_MODE_IQ))) return fail("mode %d is not KQF_MODE_DC 1, KQF_MODE_IQ 2 or both", mode);
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  long long s[6] = {0, 0, 0, 0, 0, 0};
  HIP_OK(hipMemcpyAsync(s, h->sums, sizeof s, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  h->co = solve_sums(s, mode);                  // a launch carries its coefficients by value: enqueued work keeps the old ones
  if (out) *out = h->co;
  return 0;
}

int kqf_set_coeffs(kqf_corrector* h, float dc_i, float dc_q, float c, float d) {
  if (!h) return fail("null corrector object");
  if (!(std::isfinite(dc_i) && std::isfinite(dc_q) && std::isfinite(c) && std::isfinite(d)))
    return fail("coefficients (%g, %g, %g, %g) must be finite", (double)dc_i, (double)dc_q, (double)c, (double)d);
  h->co = kqf_coeffs{dc_i, dc_q, c, d, 0, 0, 0};
  return 0;
}

int kqf_get_coeffs(kqf_corrector* h, kqf_coeffs* out) {
  if (!h) return fail("null corrector object");
  if (!out) return fail("null coefficients out pointer");
  *out = h->co;
  return 0;
}

int kqf_read_stats(kqf_corrector* h, int64_t sums[6]) {
  if (!h) return fail("null corrector object");
  if (!sums) return fail("null sums pointer");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  HIP_OK(hipMemcpyAsync(sums, h->sums, 6 * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

int kqf_stats_dev(kqf_corrector* h, int64_t** sums_dev) {
  if (!h) return fail("null corrector object");
  if (!sums_dev) return fail("null sums out pointer");
  *sums_dev = reinterpret_cast<int64_t*>(h->sums);
  return 0;
}

int kqf_clear_stats(kqf_corrector* h) {
  if (!h) return fail("null corrector object");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  HIP_OK(hipMemsetAsync(h->sums, 0, 6 * sizeof(long long), h->stream));
  h->count = 0;
  return 0;
}

int kqf_out_dev(kqf_corrector* h, void** out_dev) {
  if (!h) return fail("null corrector object");
  if (!out_dev) return fail("null out pointer");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  if (int rc = ensure_out(h)) return rc;
  *out_dev = h->out;
  return 0;
}

int kqf_kernel_info(kqf_corrector* h, int32_t* threads, int32_t* lds_bytes, int32_t* vgprs, int32_t* grid, int32_t* tile) {
  if (!h) return fail("null corrector object");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  hipFuncAttributes attr;
  HIP_OK(hipFuncGetAttributes(&attr, kernel_of(h->fmt, h->last_apply, h->last_acc)));
  if (threads) *threads = THREADS;
  if (lds_bytes) *lds_bytes = (int32_t)attr.sharedSizeBytes;
  if (vgprs) *vgprs = attr.numRegs;
  if (grid) *grid = h->last_grid ? h->last_grid : (int32_t)std::min<long long>(ceil_div(h->max_in, TILE), MAX_GRID);
  if (tile) *tile = TILE;
  return 0;
}

}  // extern "C"
