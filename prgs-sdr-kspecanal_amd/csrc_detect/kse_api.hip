// libksa_detect: host layer of include/ksa_detect.h (validation, launch planning, staging); kernels in kse_kernels.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/ksa_detect.h"
#include "kse_kernels.hpp"
#include "../csrc_shared/ksa_host.hpp"

static_assert(sizeof(kse_emission) == sizeof(ksa::detect::Emission), "kse_emission and the kernels' record are one layout");
static_assert(KSE_MODE_CA == ksa::detect::MODE_CA && KSE_MODE_GO == ksa::detect::MODE_GO && KSE_MODE_SO == ksa::detect::MODE_SO,
              "the modes of the header are the kernels'");

namespace {

constexpr long long MAX_LAUNCH_ROWS = 1ll << 20;        // bounds the per-row scratch, made at creation: 12 MiB
constexpr long long STAGE_BYTES = 64ll << 20;           // kse_detect_rows: rows cross in pieces of at most this size
constexpr int LDS_PER_CU = 160 * 1024;
constexpr int MAX_WG_PER_CU = 8;                        // 2048 threads of a CU
constexpr int WG_ROUNDS = 2;                            // workgroups per resident place: evens out rows of unequal work

struct Params {
  int train = 0, guard = 0, tq = 0, mode = 0, min_width = 1, max_gap = 0;
};

}  // namespace

struct kse_detector {
  int device = 0, nbins = 0, capacity = 0, cus = 1, group = 0, lds_bytes = 0, last_grid = 0, last_vec = -1;
  Params par;
  long long rows_seen = 0;
  long long* hits = nullptr;                    // device [nbins]
  ksa::detect::Emission* events = nullptr;      // device [capacity]
  long long* totals = nullptr;                  // device [2]: emissions_total, its snapshot
  long long* block_sums = nullptr;              // device [MAX_LAUNCH_ROWS / SCAN_THREADS]
  int* cnt = nullptr;                           // device scratch [MAX_LAUNCH_ROWS]
  long long* off = nullptr;                     // device scratch [MAX_LAUNCH_ROWS]
  float* stage = nullptr;
  long long stage_floats = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_stream = nullptr;
};

namespace {

// the detection parameters' own rules, shared by kse_create and kse_set_params
int check_params(int nbins, int train, int guard, float threshold_db, int mode, int min_width, int max_gap, Params* out) {
  if (train < 1 || train > KSE_MAX_TRAIN) return fail("train %d outside 1..%d", train, KSE_MAX_TRAIN);
  if (guard < 0 || guard > KSE_MAX_GUARD) return fail("guard %d outside 0..%d", guard, KSE_MAX_GUARD);
  if (!std::isfinite(threshold_db) || threshold_db < 0.0f || threshold_db > 100.0f)
    return fail("threshold_db %g is not a finite value in 0..100", (double)threshold_db);
  if (mode != KSE_MODE_CA && mode != KSE_MODE_GO && mode != KSE_MODE_SO)
    return fail("mode %d is none of KSE_MODE_CA 0, KSE_MODE_GO 1, KSE_MODE_SO 2", mode);
  if (min_width < 1) return fail("min_width %d must be >= 1", min_width);
  if (min_width > nbins) return fail("min_width %d exceeds the %d bins of a row", min_width, nbins);
  if (max_gap < 0 || max_gap > KSE_MAX_GAP) return fail("max_gap %d outside 0..%d", max_gap, KSE_MAX_GAP);
  out->train = train;
  out->guard = guard;
  out->tq = (int)std::rintf(threshold_db * 64.0f);
  out->mode = mode;
  out->min_width = min_width;
  out->max_gap = max_gap;
  return 0;
}

bool vec_for(const kse_detector* d, const float* rows_dev, long long row_stride) {
  return d->nbins % 4 == 0 && (reinterpret_cast<uintptr_t>(rows_dev) & 15) == 0 && row_stride % 4 == 0;
}

const void* row_fn(bool vec, bool emit) {
  using namespace ksa::detect;
  if (vec) return emit ? reinterpret_cast<const void*>(row_kernel<true, true>) : reinterpret_cast<const void*>(row_kernel<true, false>);
  return emit ? reinterpret_cast<const void*>(row_kernel<false, true>) : reinterpret_cast<const void*>(row_kernel<false, false>);
}

int rows_per_wg(const kse_detector* d) { return ksa::detect::THREADS / d->group; }

// workgroups for n rows: what the device holds at once (by LDS), WG_ROUNDS times over, never more than there are passes
int grid_for(const kse_detector* d, long long n) {
  const int resident = std::max(1, std::min(MAX_WG_PER_CU, LDS_PER_CU / std::max(1, d->lds_bytes)));
  const long long passes = (n + rows_per_wg(d) - 1) / rows_per_wg(d);
  return (int)std::max<long long>(1, std::min<long long>(passes, (long long)d->cus * resident * WG_ROUNDS));
}

// rows [0, nrows) of rows_dev, numbered from d->rows_seen; rows_seen moves with every launch that was enqueued
int launch_detect(kse_detector* d, const float* rows_dev, long long row_stride, long long nrows, int32_t* row_count_dev,
                  float* floor_dev) {
  using namespace ksa::detect;
  const bool vec = vec_for(d, rows_dev, row_stride);
  for (long long done = 0; done < nrows;) {
    const long long n = std::min(nrows - done, MAX_LAUNCH_ROWS);
    RowArgs a;
    a.rows = rows_dev + done * row_stride;
    a.row_stride = row_stride;
    a.cnt = d->cnt;
    a.off = d->off;
    a.floor_out = floor_dev ? floor_dev + done * d->nbins : nullptr;
    a.hits = reinterpret_cast<unsigned long long*>(d->hits);
    a.events = d->events;
    a.row_base = d->rows_seen;
    a.nrows = (int)n;
    a.nbins = d->nbins;
    a.group = d->group;
    a.train = d->par.train;
    a.guard = d->par.guard;
    a.tq = d->par.tq;
    a.mode = d->par.mode;
    a.min_width = d->par.min_width;
    a.max_gap = d->par.max_gap;
    a.capacity = d->capacity;
    const int grid = grid_for(d, n);
    d->last_grid = grid;
    d->last_vec = vec ? 1 : 0;
    if (vec) hipLaunchKernelGGL((row_kernel<true, false>), dim3(grid), dim3(THREADS), d->lds_bytes, d->stream, a);
    else hipLaunchKernelGGL((row_kernel<false, false>), dim3(grid), dim3(THREADS), d->lds_bytes, d->stream, a);
    HIP_OK(hipGetLastError());
    ScanArgs s;
    s.cnt = d->cnt;
    s.nrows = (int)n;
    s.row_count = row_count_dev ? row_count_dev + done : nullptr;
    s.block_sums = d->block_sums;
    s.total = d->totals;
    s.snapshot = d->totals + 1;
    s.off = d->off;
    const int blocks = (int)((n + SCAN_THREADS - 1) / SCAN_THREADS);
    hipLaunchKernelGGL(sum_kernel, dim3(blocks), dim3(SCAN_THREADS), 0, d->stream, s);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(offset_kernel, dim3(blocks), dim3(SCAN_THREADS), 0, d->stream, s);
    HIP_OK(hipGetLastError());
    if (vec) hipLaunchKernelGGL((row_kernel<true, true>), dim3(grid), dim3(THREADS), d->lds_bytes, d->stream, a);
    else hipLaunchKernelGGL((row_kernel<false, true>), dim3(grid), dim3(THREADS), d->lds_bytes, d->stream, a);
    HIP_OK(hipGetLastError());
    d->rows_seen += n;
    done += n;
  }
  return 0;
}

void free_all(kse_detector* d) {
  if (d->ev_stream) (void)hipEventDestroy(d->ev_stream);
  free_device({d->hits, d->events, d->totals, d->block_sums, d->cnt, d->off, d->stage});
  delete d;
}

}  // namespace

extern "C" {

int kse_abi_version(void) { return KSE_ABI_VERSION; }
const char* kse_last_error(void) { return g_err.c_str(); }

int kse_create(int32_t device, int32_t nbins, int32_t train, int32_t guard, float threshold_db, int32_t mode, int32_t min_width,
               int32_t max_gap, int32_t capacity, kse_detector** out) {
  if (!out) return fail("null out pointer");
  *out = nullptr;
  if (nbins < KSE_MIN_NBINS || nbins > KSE_MAX_NBINS) return fail("nbins %d outside %d..%d", nbins, KSE_MIN_NBINS, KSE_MAX_NBINS);
  Params par;
  if (int rc = check_params(nbins, train, guard, threshold_db, mode, min_width, max_gap, &par)) return rc;
  if (capacity < 1 || capacity > KSE_MAX_CAPACITY) return fail("emission capacity %d outside 1..%d", capacity, KSE_MAX_CAPACITY);
  if (check_device(device)) return 1;

  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(device));
  kse_detector* d = new kse_detector;
  d->device = device; d->nbins = nbins; d->capacity = capacity; d->par = par;
  d->group = ksa::detect::group_for(nbins);
  d->lds_bytes = ksa::detect::layout_for(nbins).slot * rows_per_wg(d);
  int rc = 0;
  do {
    if ((rc = cu_count(device, &d->cus))) break;
    hipError_t e = hipSuccess;
    const int lds_max = ksa::detect::layout_for(KSE_MAX_NBINS).slot;      // one value for every object of the process
    for (int v = 0; v < 4 && e == hipSuccess; ++v)
      e = hipFuncSetAttribute(row_fn(v & 1, v & 2), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    if (e != hipSuccess) { rc = fail("hipFuncSetAttribute(MaxDynamicSharedMemorySize, %d) failed: %s", lds_max, hipGetErrorString(e)); break; }
    const size_t hits = (size_t)nbins * 8, events = (size_t)capacity * sizeof(ksa::detect::Emission);
    const size_t sums = (size_t)(MAX_LAUNCH_ROWS / ksa::detect::SCAN_THREADS) * sizeof(long long);
    e = hipMalloc(reinterpret_cast<void**>(&d->hits), hits);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d->events), events);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d->totals), 16);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d->block_sums), sums);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d->cnt), (size_t)MAX_LAUNCH_ROWS * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d->off), (size_t)MAX_LAUNCH_ROWS * sizeof(long long));
    if (e != hipSuccess) { rc = fail("hipMalloc of the detector object's device memory failed: %s", hipGetErrorString(e)); break; }
    e = hipMemsetAsync(d->hits, 0, hits, d->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d->events, 0, events, d->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d->totals, 0, 16, d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    if (e != hipSuccess) { rc = fail("zeroing the detector object's device memory failed: %s", hipGetErrorString(e)); break; }
  } while (0);
  if (rc) {
    free_all(d);
    return rc;
  }
  *out = d;
  return 0;
}

void kse_destroy(kse_detector* d) {
  if (!d) return;
  DeviceGuard dev_guard;
  (void)hipSetDevice(d->device);
  (void)hipStreamSynchronize(d->stream);
  free_all(d);
}

int kse_set_stream(kse_detector* d, void* hip_stream) {
  if (!d) return fail("null detector object");
  return hand_over_stream(d->device, &d->stream, &d->ev_stream, hip_stream);
}

int kse_synchronize(kse_detector* d) {
  if (!d) return fail("null detector object");
  return synchronize_on(d->device, d->stream);
}

int kse_detect_rows_dev(kse_detector* d, const float* rows_dev, int64_t row_stride, int64_t nrows, int32_t* row_count_dev,
                        float* floor_dev) {
  if (!d) return fail("null detector object");
  if (!rows_dev) return fail("null rows pointer");
  if (nrows < 0) return fail("nrows %lld must be >= 0", (long long)nrows);
  if (row_stride < d->nbins) return fail("row_stride %lld is shorter than a row of %d bins", (long long)row_stride, d->nbins);
  if (reinterpret_cast<uintptr_t>(rows_dev) & 3) return fail("rows pointer is not 4-byte aligned");
  if (nrows == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(d->device));
  return launch_detect(d, rows_dev, row_stride, nrows, row_count_dev, floor_dev);
}

int kse_detect_rows(kse_detector* d, const float* rows_host, int64_t nrows) {
  if (!d) return fail("null detector object");
  if (!rows_host) return fail("null rows pointer");
  if (nrows < 0) return fail("nrows %lld must be >= 0", (long long)nrows);
  if (nrows == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(d->device));
  const long long piece = std::min(MAX_LAUNCH_ROWS, std::max<long long>(1, STAGE_BYTES / ((long long)d->nbins * 4)));
  const long long need = std::min<long long>(piece, nrows) * d->nbins;
  if (int rc = grow_device(&d->stage, &d->stage_floats, need, d->stream)) return rc;
  // the pieces queue one behind the other on the object's stream, so one staging buffer serves them all
  for (long long done = 0; done < nrows;) {
    const long long n = std::min(piece, nrows - done);
    HIP_OK(hipMemcpyAsync(d->stage, rows_host + done * d->nbins, (size_t)n * d->nbins * 4, hipMemcpyHostToDevice, d->stream));
    if (int rc = launch_detect(d, d->stage, d->nbins, n, nullptr, nullptr)) return rc;
    done += n;
  }
  HIP_OK(hipStreamSynchronize(d->stream));
  return 0;
}

int kse_set_params(kse_detector* d, int32_t train, int32_t guard, float threshold_db, int32_t mode, int32_t min_width,
                   int32_t max_gap) {
  if (!d) return fail("null detector object");
  Params par;
  if (int rc = check_params(d->nbins, train, guard, threshold_db, mode, min_width, max_gap, &par)) return rc;
  d->par = par;                                 // a launch carries its parameters by value: enqueued rows keep the old ones
  return 0;
}

int kse_set_row_base(kse_detector* d, int64_t row_base) {
  if (!d) return fail("null detector object");
  if (row_base < 0) return fail("row base %lld must be >= 0", (long long)row_base);
  d->rows_seen = row_base;
  return 0;
}

int kse_read_hits(kse_detector* d, int64_t* hits_host, int64_t* rows_seen) {
  if (!d) return fail("null detector object");
  if (!hits_host && !rows_seen) return fail("null hits and rows_seen pointers");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(d->device));
  if (hits_host) HIP_OK(hipMemcpyAsync(hits_host, d->hits, (size_t)d->nbins * 8, hipMemcpyDeviceToHost, d->stream));
  HIP_OK(hipStreamSynchronize(d->stream));
  if (rows_seen) *rows_seen = d->rows_seen;
  return 0;
}

int kse_read_emissions(kse_detector* d, void* records_host, int64_t max_records, int64_t* stored, int64_t* total) {
  if (!d) return fail("null detector object");
  if (max_records < 0) return fail("max_records %lld must be >= 0", (long long)max_records);
  if (!records_host && !stored && !total) return fail("null records, stored and total pointers");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(d->device));
  long long all = 0;
  HIP_OK(hipMemcpyAsync(&all, d->totals, 8, hipMemcpyDeviceToHost, d->stream));
  HIP_OK(hipStreamSynchronize(d->stream));
  const long long kept = std::min<long long>(all, d->capacity);
  const long long n = records_host ? std::min<long long>(kept, max_records) : 0;
  if (n > 0) {
    HIP_OK(hipMemcpyAsync(records_host, d->events, (size_t)n * sizeof(kse_emission), hipMemcpyDeviceToHost, d->stream));
    HIP_OK(hipStreamSynchronize(d->stream));
  }
  if (stored) *stored = kept;
  if (total) *total = all;
  return 0;
}

int kse_hits_dev(kse_detector* d, int64_t** hits_dev) {
  if (!d) return fail("null detector object");
  if (!hits_dev) return fail("null out pointer");
  *hits_dev = reinterpret_cast<int64_t*>(d->hits);
  return 0;
}

int kse_emissions_dev(kse_detector* d, void** records_dev, int64_t** emissions_total_dev) {
  if (!d) return fail("null detector object");
  if (!records_dev && !emissions_total_dev) return fail("null records and emissions_total out pointers");
  if (records_dev) *records_dev = d->events;
  if (emissions_total_dev) *emissions_total_dev = reinterpret_cast<int64_t*>(d->totals);
  return 0;
}

int kse_merge_hits_dev(kse_detector* d, const int64_t* hits_dev, int64_t rows_seen_add) {
  if (!d) return fail("null detector object");
  if (!hits_dev) return fail("null hits pointer");
  if (rows_seen_add < 0) return fail("rows_seen_add %lld must be >= 0", (long long)rows_seen_add);
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(d->device));
  const long long n = d->nbins;
  const int grid = (int)std::min<long long>((n + 255) / 256, (long long)d->cus * 8);
  hipLaunchKernelGGL(ksa::detect::merge_kernel, dim3(grid), dim3(256), 0, d->stream, d->hits,
                     reinterpret_cast<const long long*>(hits_dev), n);
  HIP_OK(hipGetLastError());
  d->rows_seen += rows_seen_add;
  return 0;
}

int kse_clear_emissions(kse_detector* d) {
  if (!d) return fail("null detector object");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(d->device));
  HIP_OK(hipMemsetAsync(d->events, 0, (size_t)d->capacity * sizeof(ksa::detect::Emission), d->stream));
  HIP_OK(hipMemsetAsync(d->totals, 0, 16, d->stream));
  return 0;
}

int kse_reset(kse_detector* d) {
  if (!d) return fail("null detector object");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(d->device));
  HIP_OK(hipMemsetAsync(d->hits, 0, (size_t)d->nbins * 8, d->stream));
  HIP_OK(hipMemsetAsync(d->events, 0, (size_t)d->capacity * sizeof(ksa::detect::Emission), d->stream));
  HIP_OK(hipMemsetAsync(d->totals, 0, 16, d->stream));
  d->rows_seen = 0;
  return 0;
}

int kse_kernel_info(kse_detector* d, int32_t* threads, int32_t* lds_bytes, int32_t* vgprs, int32_t* grid, int32_t* vec,
                    int32_t* rows_per_wg_out) {
  if (!d) return fail("null detector object");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(d->device));
  const bool v = d->last_vec >= 0 ? d->last_vec == 1 : d->nbins % 4 == 0;
  hipFuncAttributes attr;
  HIP_OK(hipFuncGetAttributes(&attr, row_fn(v, false)));
  if (threads) *threads = ksa::detect::THREADS;
  if (lds_bytes) *lds_bytes = d->lds_bytes + (int32_t)attr.sharedSizeBytes;
  if (vgprs) *vgprs = attr.numRegs;
  if (grid) *grid = d->last_grid ? d->last_grid : grid_for(d, 1ll << 40);
  if (vec) *vec = v ? 1 : 0;
  if (rows_per_wg_out) *rows_per_wg_out = rows_per_wg(d);
  return 0;
}

}  // extern "C"
