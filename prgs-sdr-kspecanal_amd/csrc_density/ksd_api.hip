// libksa_density: host layer of include/ksa_density.h (validation, launch planning, staging); kernels in ksd_kernels.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/ksa_density.h"
#include "ksd_kernels.hpp"
#include "../csrc_shared/ksa_host.hpp"

namespace {

constexpr int LDS_PLAIN = 64 << 10;       // dynamic LDS a kernel gets without asking
constexpr int LDS_OPTIN = 128 << 10;      // what a strip may grow to when it would otherwise be narrower than 64 bytes of a row
constexpr int MIN_STRIP_BINS = 16;
constexpr int MAX_CHUNK_ROWS = 1 << 16;
constexpr int MIN_CHUNK_ROWS = 8;         // below this a workgroup's LDS clear and flush outweigh its rows
constexpr int WG_PER_CU = 4;              // workgroups per CU that a launch aims for
constexpr long long MAX_GRID = 1ll << 24;
constexpr long long STAGE_BYTES = 64ll << 20;   // ksd_add_rows: rows cross in pieces of at most this size

using AddFn = void (*)(const ksa::density::AddArgs);

AddFn add_fn(bool vec, bool combine) {
  using namespace ksa::density;
  return vec ? (combine ? add_kernel<true, true> : add_kernel<true, false>)
             : (combine ? add_kernel<false, true> : add_kernel<false, false>);
}

}  // namespace

struct ksd_density {
  int device = 0, nbins = 0, W = 0, L = 0, g = 1;
  float lo = 0, hi = 0, inv = 0;
  int S = 1, pitch = 1, nstrips = 1, lds_bytes = 0, cus = 1, last_grid = 0;
  bool vec_shape = false;               // strips start and end on 16-byte boundaries of an aligned row
  long long cells = 0, rows_seen = 0;
  long long* counts = nullptr;
  float* stage = nullptr;
  long long stage_floats = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_stream = nullptr;
};

namespace {

int elementwise_grid(const ksd_density* d) {
  return (int)std::min<long long>((d->cells + 255) / 256, (long long)d->cus * 8);
}

// chunks of rows for one launch over n rows: enough workgroups to fill the device, never more rows than uint32 cells allow
void plan_chunks(const ksd_density* d, long long n, int* chunk_rows, int* nchunks) {
  const long long cap = std::min<long long>(MAX_CHUNK_ROWS, 0xFFFFFFFFll / d->g);
  long long want = std::max<long long>(1, ((long long)d->cus * WG_PER_CU + d->nstrips - 1) / d->nstrips);
  want = std::min(want, std::max<long long>(1, n / MIN_CHUNK_ROWS));
  long long rows = std::min(cap, (n + want - 1) / want);
  *chunk_rows = (int)rows;
  *nchunks = (int)((n + rows - 1) / rows);
}

int launch_add(ksd_density* d, const float* rows_dev, long long row_stride, long long nrows) {
  const bool vec = d->vec_shape && (reinterpret_cast<uintptr_t>(rows_dev) & 15) == 0 && row_stride % 4 == 0;
  const AddFn fn = add_fn(vec, d->g > 1);
  const long long cap = std::min<long long>(MAX_CHUNK_ROWS, 0xFFFFFFFFll / d->g);
  const long long per_launch = std::max<long long>(1, MAX_GRID / d->nstrips) * cap;
  for (long long done = 0; done < nrows;) {
    const long long n = std::min(nrows - done, std::min<long long>(per_launch, INT32_MAX));
    ksa::density::AddArgs a;
    a.rows = rows_dev + done * row_stride;
    a.row_stride = row_stride;
    a.counts = reinterpret_cast<unsigned long long*>(d->counts);
    a.nrows = (int)n;
    a.W = d->W; a.g = d->g; a.L = d->L; a.S = d->S; a.pitch = d->pitch; a.nstrips = d->nstrips;
    a.lo = d->lo; a.inv = d->inv;
    int nchunks = 1;
    plan_chunks(d, n, &a.chunk_rows, &nchunks);
    d->last_grid = d->nstrips * nchunks;
    hipLaunchKernelGGL(fn, dim3(d->last_grid), dim3(ksa::density::THREADS), d->lds_bytes, d->stream, a);
    HIP_OK(hipGetLastError());
    done += n;
  }
  return 0;
}

}  // namespace

extern "C" {

int ksd_abi_version(void) { return KSD_ABI_VERSION; }
const char* ksd_last_error(void) { return g_err.c_str(); }

int ksd_create(int32_t device, int32_t nbins, int32_t width, int32_t levels, float lo_db, float hi_db, ksd_density** out) {
  if (!out) return fail("null out pointer");
  *out = nullptr;
  if (nbins < KSD_MIN_NBINS || nbins > KSD_MAX_NBINS) return fail("nbins %d outside %d..%d", nbins, KSD_MIN_NBINS, KSD_MAX_NBINS);
  if (width < 1) return fail("width %d must be >= 1", width);
  if (nbins % width) return fail("width %d does not divide nbins %d", width, nbins);
  if (levels < 1 || levels > KSD_MAX_LEVELS) return fail("levels %d outside 1..%d", levels, KSD_MAX_LEVELS);
  if (!std::isfinite(lo_db) || !std::isfinite(hi_db)) return fail("level range [%g, %g) is not finite", lo_db, hi_db);
  if (!(lo_db < hi_db)) return fail("level range needs lo_db %g < hi_db %g", lo_db, hi_db);
  const float span = hi_db - lo_db;                   // one subtraction, one division, both rounded to float32
  const float inv = (float)levels / span;
  if (!std::isfinite(span) || !std::isfinite(inv) || !(inv > 0.0f))
    return fail("levels / (hi_db - lo_db) = %d / (%g - %g) is not a finite positive float32", levels, hi_db, lo_db);
  const long long cells = (long long)(levels + 1) * width;
  if (cells > KSD_MAX_CELLS) return fail("(levels + 1) * width = %lld exceeds %d cells (1 GiB of counters)", cells, KSD_MAX_CELLS);
  if (check_device(device)) return 1;

  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(device));
  ksd_density* d = new ksd_density;
  d->device = device; d->nbins = nbins; d->W = width; d->L = levels; d->g = nbins / width;
  d->lo = lo_db; d->hi = hi_db; d->inv = inv; d->cells = cells;
  // strip width: the widest power of two whose [L+1][S|1] uint32 partials fit the plain LDS limit; a strip narrower than 64
  // bytes of a row (L = 1024 at g = 1) may double into the opt-in range
  int S = 1;
  while (S * 2 <= width && (long long)(levels + 1) * ((S * 2) | 1) * 4 <= LDS_PLAIN) S *= 2;
  while ((long long)S * d->g < MIN_STRIP_BINS && S * 2 <= width && (long long)(levels + 1) * ((S * 2) | 1) * 4 <= LDS_OPTIN) S *= 2;
  if (S * 2 > width && (long long)(levels + 1) * (width | 1) * 4 <= LDS_PLAIN) S = width;     // one strip takes a non-power-of-two width whole
  d->S = S;
  d->pitch = S | 1;
  d->nstrips = (width + S - 1) / S;
  d->lds_bytes = (levels + 1) * d->pitch * 4;
  d->vec_shape = nbins % 4 == 0 && (d->nstrips == 1 || ((long long)S * d->g) % 4 == 0);
  int rc = 0;
  do {
    if ((rc = cu_count(device, &d->cus))) break;
    if (d->lds_bytes > LDS_PLAIN) {
      for (int v = 0; v < 4 && !rc; ++v)
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(add_fn(v & 1, v & 2)), hipFuncAttributeMaxDynamicSharedMemorySize,
                                d->lds_bytes) != hipSuccess)
          rc = fail("the add kernel was refused %d bytes of LDS", d->lds_bytes);
      if (rc) break;
    }
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d->counts), (size_t)cells * 8);
    if (e != hipSuccess) { rc = fail("hipMalloc of %lld counter bytes failed: %s", cells * 8, hipGetErrorString(e)); break; }
    e = hipMemsetAsync(d->counts, 0, (size_t)cells * 8, d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    if (e != hipSuccess) { rc = fail("zeroing the counters failed: %s", hipGetErrorString(e)); break; }
  } while (0);
  if (rc) {
    free_device({d->counts});
    delete d;
    return rc;
  }
  *out = d;
  return 0;
}

void ksd_destroy(ksd_density* d) {
  if (!d) return;
  DeviceGuard dev_guard;
  (void)hipSetDevice(d->device);
  (void)hipStreamSynchronize(d->stream);
  if (d->ev_stream) (void)hipEventDestroy(d->ev_stream);
  free_device({d->counts, d->stage});
  delete d;
}

int ksd_set_stream(ksd_density* d, void* hip_stream) {
  if (!d) return fail("null density object");
  return hand_over_stream(d->device, &d->stream, &d->ev_stream, hip_stream);
}

int ksd_synchronize(ksd_density* d) {
  if (!d) return fail("null density object");
  return synchronize_on(d->device, d->stream);
}

int ksd_add_rows_dev(ksd_density* d, const float* rows_dev, int64_t row_stride, int64_t nrows) {
  if (!d) return fail("null density object");
  if (!rows_dev) return fail("null rows pointer");
  if (nrows < 0) return fail("nrows %lld must be >= 0", (long long)nrows);
  if (row_stride < d->nbins) return fail("row_stride %lld is shorter than a row of %d bins", (long long)row_stride, d->nbins);
  if (reinterpret_cast<uintptr_t>(rows_dev) & 3) return fail("rows pointer is not 4-byte aligned");
  if (nrows == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(d->device));
  if (int rc = launch_add(d, rows_dev, row_stride, nrows)) return rc;
  d->rows_seen += nrows;
  return 0;
}

int ksd_add_rows(ksd_density* d, const float* rows_host, int64_t nrows) {
  if (!d) return fail("null density object");
  if (!rows_host) return fail("null rows pointer");
  if (nrows < 0) return fail("nrows %lld must be >= 0", (long long)nrows);
  if (nrows == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(d->device));
  const long long piece = std::max<long long>(1, STAGE_BYTES / ((long long)d->nbins * 4));
  const long long need = std::min<long long>(piece, nrows) * d->nbins;
  if (int rc = grow_device(&d->stage, &d->stage_floats, need, d->stream)) return rc;
  // the pieces queue one behind the other on the object's stream, so one staging buffer serves them all; rows_seen moves
  // with every piece that was enqueued
  for (long long done = 0; done < nrows;) {
    const long long n = std::min(piece, nrows - done);
    HIP_OK(hipMemcpyAsync(d->stage, rows_host + done * d->nbins, (size_t)n * d->nbins * 4, hipMemcpyHostToDevice, d->stream));
    if (int rc = launch_add(d, d->stage, d->nbins, n)) return rc;
    d->rows_seen += n;
    done += n;
  }
  HIP_OK(hipStreamSynchronize(d->stream));
  return 0;
}

int ksd_decay(ksd_density* d, int64_t num, int64_t den) {
  if (!d) return fail("null density object");
  if (den < 1 || den > INT32_MAX) return fail("decay den %lld outside 1..2^31-1", (long long)den);
  if (num < 0 || num > den) return fail("decay num %lld outside 0..den (%lld)", (long long)num, (long long)den);
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(d->device));
  hipLaunchKernelGGL(ksa::density::decay_kernel, dim3(elementwise_grid(d)), dim3(256), 0, d->stream, d->counts, d->cells,
                     (long long)num, (long long)den);
  HIP_OK(hipGetLastError());
  return 0;
}

int ksd_merge_dev(ksd_density* d, const int64_t* counts_dev, int64_t rows_seen_add) {
  if (!d) return fail("null density object");
  if (!counts_dev) return fail("null counts pointer");
  if (rows_seen_add < 0) return fail("rows_seen_add %lld must be >= 0", (long long)rows_seen_add);
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(d->device));
  hipLaunchKernelGGL(ksa::density::merge_kernel, dim3(elementwise_grid(d)), dim3(256), 0, d->stream, d->counts,
                     reinterpret_cast<const long long*>(counts_dev), d->cells);
  HIP_OK(hipGetLastError());
  d->rows_seen += rows_seen_add;
  return 0;
}

int ksd_reset(ksd_density* d) {
  if (!d) return fail("null density object");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(d->device));
  hipLaunchKernelGGL(ksa::density::reset_kernel, dim3(elementwise_grid(d)), dim3(256), 0, d->stream, d->counts, d->cells);
  HIP_OK(hipGetLastError());
  d->rows_seen = 0;
  return 0;
}

int ksd_read(ksd_density* d, int64_t* counts_host, int64_t* rows_seen) {
  if (!d) return fail("null density object");
  if (!counts_host && !rows_seen) return fail("null counts and rows_seen pointers");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(d->device));
  if (counts_host) HIP_OK(hipMemcpyAsync(counts_host, d->counts, (size_t)d->cells * 8, hipMemcpyDeviceToHost, d->stream));
  HIP_OK(hipStreamSynchronize(d->stream));
  if (rows_seen) *rows_seen = d->rows_seen;
  return 0;
}

int ksd_counts_dev(ksd_density* d, int64_t** counts_dev) {
  if (!d) return fail("null density object");
  if (!counts_dev) return fail("null out pointer");
  *counts_dev = reinterpret_cast<int64_t*>(d->counts);
  return 0;
}

int ksd_kernel_info(ksd_density* d, int32_t* threads, int32_t* lds_bytes, int32_t* vgprs, int32_t* grid, int32_t* strip_cols,
                    int32_t* lds_optin) {
  if (!d) return fail("null density object");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(d->device));
  hipFuncAttributes attr;
  HIP_OK(hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(add_fn(d->vec_shape, d->g > 1))));
  const int nominal_chunks = std::max(1, (d->cus * WG_PER_CU + d->nstrips - 1) / d->nstrips);
  if (threads) *threads = ksa::density::THREADS;
  if (lds_bytes) *lds_bytes = d->lds_bytes;
  if (vgprs) *vgprs = attr.numRegs;
  if (grid) *grid = d->last_grid ? d->last_grid : d->nstrips * nominal_chunks;
  if (strip_cols) *strip_cols = d->S;
  if (lds_optin) *lds_optin = d->lds_bytes > LDS_PLAIN ? 1 : 0;
  return 0;
}

}  // extern "C"
