// libksa_mask: host layer of include/ksa_mask.h (validation, launch planning, staging); kernels in ksm_kernels.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "../../include/ksa_mask.h"
#include "ksm_kernels.hpp"
#include "../csrc_shared/ksa_host.hpp"

static_assert(sizeof(ksm_event) == sizeof(ksa::mask::Event), "ksm_event and the kernels' record are one layout");

namespace {

constexpr int MAX_CHUNK_ROWS = 1 << 16;         // a lane's uint32 hit counters cannot wrap
constexpr int MIN_CHUNK_ROWS = 8;               // below this a workgroup's line loads and flush outweigh its rows
constexpr int WG_PER_CU = 4;                    // workgroups per CU that a launch aims for
constexpr long long MAX_LAUNCH_ROWS = 1ll << 20;        // bounds the per-row scratch: 24 MiB
constexpr long long STAGE_BYTES = 64ll << 20;   // ksm_check_rows: rows cross in pieces of at most this size

}  // namespace

struct ksm_mask {
  int device = 0, nbins = 0, min_bins = 1, capacity = 0, cus = 1, last_grid = 0, last_vec = -1;
  long long rows_seen = 0;
  float* upper = nullptr;                       // device [nbins]
  float* lower = nullptr;                       // device [nbins]
  long long* hits = nullptr;                    // device [3][nbins]
  ksa::mask::Event* events = nullptr;           // device [capacity]
  long long* totals = nullptr;                  // device [2]: events_total, its snapshot
  int* block_counts = nullptr;                  // device [MAX_LAUNCH_ROWS / SCAN_THREADS]
  ksa::mask::RowRec* rec = nullptr;             // device scratch [rec_rows]
  long long rec_rows = 0;
  float* stage = nullptr;
  long long stage_floats = 0;
  std::vector<float> no_lower;                  // host [nbins] of -inf, for a NULL lower line
  hipStream_t stream = nullptr;
  hipEvent_t ev_stream = nullptr;
};

namespace {

// the lines' own rules: no NaN, lower <= upper.  lower may be null.
int check_lines(int nbins, const float* upper, const float* lower) {
  if (!upper) return fail("null upper line");
  for (int b = 0; b < nbins; ++b) {
    if (std::isnan(upper[b])) return fail("upper[%d] is NaN", b);
    if (lower && std::isnan(lower[b])) return fail("lower[%d] is NaN", b);
    if (lower && lower[b] > upper[b]) return fail("lower[%d] = %g lies above upper[%d] = %g", b, lower[b], b, upper[b]);
  }
  return 0;
}

int upload_lines(ksm_mask* m, const float* upper, const float* lower) {
  const size_t bytes = (size_t)m->nbins * 4;
  HIP_OK(hipMemcpyAsync(m->upper, upper, bytes, hipMemcpyHostToDevice, m->stream));
  HIP_OK(hipMemcpyAsync(m->lower, lower ? lower : m->no_lower.data(), bytes, hipMemcpyHostToDevice, m->stream));
  HIP_OK(hipStreamSynchronize(m->stream));
  return 0;
}

bool vec_for(const ksm_mask* m, const float* rows_dev, long long row_stride) {
  return m->nbins % 4 == 0 && (reinterpret_cast<uintptr_t>(rows_dev) & 15) == 0 && row_stride % 4 == 0;
}

int strips_of(const ksm_mask* m, bool vec) {
  const int sb = ksa::mask::THREADS * (vec ? 4 : 1);
  return (m->nbins + sb - 1) / sb;
}

// chunks of rows for one launch over n rows: enough workgroups to fill the device, never more rows than a chunk may hold
void plan_chunks(const ksm_mask* m, int nstrips, long long n, int* chunk_rows, int* nchunks) {
  long long want = std::max<long long>(1, ((long long)m->cus * WG_PER_CU + nstrips - 1) / nstrips);
  want = std::min(want, std::max<long long>(1, n / MIN_CHUNK_ROWS));
  const long long rows = std::min<long long>(MAX_CHUNK_ROWS, (n + want - 1) / want);
  *chunk_rows = (int)rows;
  *nchunks = (int)((n + rows - 1) / rows);
}

// rows [0, nrows) of rows_dev, numbered from m->rows_seen; rows_seen moves with every launch that was enqueued
int launch_check(ksm_mask* m, const float* rows_dev, long long row_stride, long long nrows, uint8_t* row_event_dev) {
  using namespace ksa::mask;
  const bool vec = vec_for(m, rows_dev, row_stride);
  const int nstrips = strips_of(m, vec);
  if (int rc = grow_device(&m->rec, &m->rec_rows, std::min(nrows, MAX_LAUNCH_ROWS), m->stream)) return rc;
  for (long long done = 0; done < nrows;) {
    const long long n = std::min(nrows - done, MAX_LAUNCH_ROWS);
    HIP_OK(hipMemsetAsync(m->rec, 0, (size_t)n * sizeof(RowRec), m->stream));
    CheckArgs a;
    a.rows = rows_dev + done * row_stride;
    a.row_stride = row_stride;
    a.upper = m->upper;
    a.lower = m->lower;
    a.hits = reinterpret_cast<unsigned long long*>(m->hits);
    a.rec = m->rec;
    a.nrows = (int)n;
    a.nbins = m->nbins;
    a.nstrips = nstrips;
    int nchunks = 1;
    plan_chunks(m, nstrips, n, &a.chunk_rows, &nchunks);
    m->last_grid = nstrips * nchunks;
    m->last_vec = vec ? 1 : 0;
    if (vec) hipLaunchKernelGGL(check_kernel<true>, dim3(m->last_grid), dim3(THREADS), 0, m->stream, a);
    else hipLaunchKernelGGL(check_kernel<false>, dim3(m->last_grid), dim3(THREADS), 0, m->stream, a);
    HIP_OK(hipGetLastError());
    ScanArgs s;
    s.rec = m->rec;
    s.nrows = (int)n;
    s.min_bins = m->min_bins;
    s.capacity = m->capacity;
    s.row_event = row_event_dev ? row_event_dev + done : nullptr;
    s.block_counts = m->block_counts;
    s.events_total = m->totals;
    s.snapshot = m->totals + 1;
    s.events = m->events;
    s.row_base = m->rows_seen;
    const int blocks = (int)((n + SCAN_THREADS - 1) / SCAN_THREADS);
    hipLaunchKernelGGL(count_kernel, dim3(blocks), dim3(SCAN_THREADS), 0, m->stream, s);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(scatter_kernel, dim3(blocks), dim3(SCAN_THREADS), 0, m->stream, s);
    HIP_OK(hipGetLastError());
    m->rows_seen += n;
    done += n;
  }
  return 0;
}

void free_all(ksm_mask* m) {
  if (m->ev_stream) (void)hipEventDestroy(m->ev_stream);
  free_device({m->upper, m->lower, m->hits, m->events, m->totals, m->block_counts, m->rec, m->stage});
  delete m;
}

}  // namespace

extern "C" {

int ksm_abi_version(void) { return KSM_ABI_VERSION; }
const char* ksm_last_error(void) { return g_err.c_str(); }

int ksm_create(int32_t device, int32_t nbins, const float* upper_host, const float* lower_host, int32_t min_bins,
               int32_t capacity, ksm_mask** out) {
  if (!out) return fail("null out pointer");
  *out = nullptr;
  if (nbins < KSM_MIN_NBINS || nbins > KSM_MAX_NBINS) return fail("nbins %d outside %d..%d", nbins, KSM_MIN_NBINS, KSM_MAX_NBINS);
  if (min_bins < 1) return fail("min_bins %d must be >= 1", min_bins);
  if (min_bins > nbins) return fail("min_bins %d exceeds the %d bins of a row", min_bins, nbins);
  if (capacity < 1 || capacity > KSM_MAX_CAPACITY) return fail("event capacity %d outside 1..%d", capacity, KSM_MAX_CAPACITY);
  if (int rc = check_lines(nbins, upper_host, lower_host)) return rc;
  if (check_device(device)) return 1;

  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(device));
  ksm_mask* m = new ksm_mask;
  m->device = device; m->nbins = nbins; m->min_bins = min_bins; m->capacity = capacity;
  m->no_lower.assign((size_t)nbins, -std::numeric_limits<float>::infinity());
  int rc = 0;
  do {
    if ((rc = cu_count(device, &m->cus))) break;
    const size_t line = (size_t)nbins * 4, events = (size_t)capacity * sizeof(ksa::mask::Event);
    const size_t counts = (size_t)(MAX_LAUNCH_ROWS / ksa::mask::SCAN_THREADS) * sizeof(int);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&m->upper), line);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&m->lower), line);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&m->hits), line * 6);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&m->events), events);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&m->totals), 16);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&m->block_counts), counts);
    if (e != hipSuccess) { rc = fail("hipMalloc of the mask object's device memory failed: %s", hipGetErrorString(e)); break; }
    e = hipMemsetAsync(m->hits, 0, line * 6, m->stream);
    if (e == hipSuccess) e = hipMemsetAsync(m->events, 0, events, m->stream);
    if (e == hipSuccess) e = hipMemsetAsync(m->totals, 0, 16, m->stream);
    if (e != hipSuccess) { rc = fail("zeroing the mask object's device memory failed: %s", hipGetErrorString(e)); break; }
    rc = upload_lines(m, upper_host, lower_host);
  } while (0);
  if (rc) {
    free_all(m);
    return rc;
  }
  *out = m;
  return 0;
}

void ksm_destroy(ksm_mask* m) {
  if (!m) return;
  DeviceGuard dev_guard;
  (void)hipSetDevice(m->device);
  (void)hipStreamSynchronize(m->stream);
  free_all(m);
}

int ksm_set_stream(ksm_mask* m, void* hip_stream) {
  if (!m) return fail("null mask object");
  return hand_over_stream(m->device, &m->stream, &m->ev_stream, hip_stream);
}

int ksm_synchronize(ksm_mask* m) {
  if (!m) return fail("null mask object");
  return synchronize_on(m->device, m->stream);
}

int ksm_check_rows_dev(ksm_mask* m, const float* rows_dev, int64_t row_stride, int64_t nrows, uint8_t* row_event_dev) {
  if (!m) return fail("null mask object");
  if (!rows_dev) return fail("null rows pointer");
  if (nrows < 0) return fail("nrows %lld must be >= 0", (long long)nrows);
  if (row_stride < m->nbins) return fail("row_stride %lld is shorter than a row of %d bins", (long long)row_stride, m->nbins);
  if (reinterpret_cast<uintptr_t>(rows_dev) & 3) return fail("rows pointer is not 4-byte aligned");
  if (nrows == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(m->device));
  return launch_check(m, rows_dev, row_stride, nrows, row_event_dev);
}

int ksm_check_rows(ksm_mask* m, const float* rows_host, int64_t nrows) {
  if (!m) return fail("null mask object");
  if (!rows_host) return fail("null rows pointer");
  if (nrows < 0) return fail("nrows %lld must be >= 0", (long long)nrows);
  if (nrows == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(m->device));
  const long long piece = std::min(MAX_LAUNCH_ROWS, std::max<long long>(1, STAGE_BYTES / ((long long)m->nbins * 4)));
  const long long need = std::min<long long>(piece, nrows) * m->nbins;
  if (int rc = grow_device(&m->stage, &m->stage_floats, need, m->stream)) return rc;
  // the pieces queue one behind the other on the object's stream, so one staging buffer serves them all
  for (long long done = 0; done < nrows;) {
    const long long n = std::min(piece, nrows - done);
    HIP_OK(hipMemcpyAsync(m->stage, rows_host + done * m->nbins, (size_t)n * m->nbins * 4, hipMemcpyHostToDevice, m->stream));
    if (int rc = launch_check(m, m->stage, m->nbins, n, nullptr)) return rc;
    done += n;
  }
  HIP_OK(hipStreamSynchronize(m->stream));
  return 0;
}

int ksm_set_mask(ksm_mask* m, const float* upper_host, const float* lower_host) {
  if (!m) return fail("null mask object");
  if (int rc = check_lines(m->nbins, upper_host, lower_host)) return rc;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(m->device));
  return upload_lines(m, upper_host, lower_host);
}

int ksm_set_row_base(ksm_mask* m, int64_t row_base) {
  if (!m) return fail("null mask object");
  if (row_base < 0) return fail("row base %lld must be >= 0", (long long)row_base);
  m->rows_seen = row_base;
  return 0;
}

int ksm_read_hits(ksm_mask* m, int64_t* hits_host, int64_t* rows_seen) {
  if (!m) return fail("null mask object");
  if (!hits_host && !rows_seen) return fail("null hits and rows_seen pointers");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(m->device));
  if (hits_host) HIP_OK(hipMemcpyAsync(hits_host, m->hits, (size_t)m->nbins * 24, hipMemcpyDeviceToHost, m->stream));
  HIP_OK(hipStreamSynchronize(m->stream));
  if (rows_seen) *rows_seen = m->rows_seen;
  return 0;
}

int ksm_read_events(ksm_mask* m, void* records_host, int64_t max_records, int64_t* stored, int64_t* total) {
  if (!m) return fail("null mask object");
  if (max_records < 0) return fail("max_records %lld must be >= 0", (long long)max_records);
  if (!records_host && !stored && !total) return fail("null records, stored and total pointers");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(m->device));
  long long all = 0;
  HIP_OK(hipMemcpyAsync(&all, m->totals, 8, hipMemcpyDeviceToHost, m->stream));
  HIP_OK(hipStreamSynchronize(m->stream));
  const long long kept = std::min<long long>(all, m->capacity);
  const long long n = records_host ? std::min<long long>(kept, max_records) : 0;
  if (n > 0) {
    HIP_OK(hipMemcpyAsync(records_host, m->events, (size_t)n * sizeof(ksm_event), hipMemcpyDeviceToHost, m->stream));
    HIP_OK(hipStreamSynchronize(m->stream));
  }
  if (stored) *stored = kept;
  if (total) *total = all;
  return 0;
}

int ksm_hits_dev(ksm_mask* m, int64_t** hits_dev) {
  if (!m) return fail("null mask object");
  if (!hits_dev) return fail("null out pointer");
  *hits_dev = reinterpret_cast<int64_t*>(m->hits);
  return 0;
}

int ksm_events_dev(ksm_mask* m, void** records_dev, int64_t** events_total_dev) {
  if (!m) return fail("null mask object");
  if (!records_dev && !events_total_dev) return fail("null records and events_total out pointers");
  if (records_dev) *records_dev = m->events;
  if (events_total_dev) *events_total_dev = reinterpret_cast<int64_t*>(m->totals);
  return 0;
}

int ksm_merge_hits_dev(ksm_mask* m, const int64_t* hits_dev, int64_t rows_seen_add) {
  if (!m) return fail("null mask object");
  if (!hits_dev) return fail("null hits pointer");
  if (rows_seen_add < 0) return fail("rows_seen_add %lld must be >= 0", (long long)rows_seen_add);
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(m->device));
  const long long n = 3ll * m->nbins;
  const int grid = (int)std::min<long long>((n + 255) / 256, (long long)m->cus * 8);
  hipLaunchKernelGGL(ksa::mask::merge_kernel, dim3(grid), dim3(256), 0, m->stream, m->hits,
                     reinterpret_cast<const long long*>(hits_dev), n);
  HIP_OK(hipGetLastError());
  m->rows_seen += rows_seen_add;
  return 0;
}

int ksm_clear_events(ksm_mask* m) {
  if (!m) return fail("null mask object");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(m->device));
  HIP_OK(hipMemsetAsync(m->events, 0, (size_t)m->capacity * sizeof(ksa::mask::Event), m->stream));
  HIP_OK(hipMemsetAsync(m->totals, 0, 16, m->stream));
  return 0;
}

int ksm_reset(ksm_mask* m) {
  if (!m) return fail("null mask object");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(m->device));
  HIP_OK(hipMemsetAsync(m->hits, 0, (size_t)m->nbins * 24, m->stream));
  HIP_OK(hipMemsetAsync(m->events, 0, (size_t)m->capacity * sizeof(ksa::mask::Event), m->stream));
  HIP_OK(hipMemsetAsync(m->totals, 0, 16, m->stream));
  m->rows_seen = 0;
  return 0;
}

int ksm_kernel_info(ksm_mask* m, int32_t* threads, int32_t* lds_bytes, int32_t* vgprs, int32_t* grid, int32_t* vec) {
  if (!m) return fail("null mask object");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(m->device));
  const bool v = m->last_vec >= 0 ? m->last_vec == 1 : m->nbins % 4 == 0;
  hipFuncAttributes attr;
  HIP_OK(hipFuncGetAttributes(&attr, v ? reinterpret_cast<const void*>(ksa::mask::check_kernel<true>)
                                       : reinterpret_cast<const void*>(ksa::mask::check_kernel<false>)));
  const int nstrips = strips_of(m, v);
  if (threads) *threads = ksa::mask::THREADS;
  if (lds_bytes) *lds_bytes = (int32_t)attr.sharedSizeBytes;
  if (vgprs) *vgprs = attr.numRegs;
  if (grid) *grid = m->last_grid ? m->last_grid : nstrips * std::max(1, (m->cus * WG_PER_CU + nstrips - 1) / nstrips);
  if (vec) *vec = v ? 1 : 0;
  return 0;
}

}  // extern "C"
