// libksa_track: host layer of include/ksa_track.h (validation, launch planning, staging); kernels in ktr_kernels.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/ksa_track.h"
#include "ktr_kernels.hpp"
#include "../csrc_shared/ksa_host.hpp"

static_assert(sizeof(ktr_span) == sizeof(ksa::track::Span) && sizeof(ktr_track) == sizeof(ksa::track::Track),
              "the header's records and the kernels' are one layout");
static_assert(offsetof(ktr_track, bin_lo) == 40 && offsetof(ktr_track, first_span) == 64 && offsetof(ktr_track, peak_db) == 72,
              "ktr_track has no padding");
static_assert(KTR_FLAG_OPEN_END == ksa::track::FLAG_OPEN_END, "the flag of the header is the kernels'");

namespace {

struct Params {
  int row_gap = 0, bin_slop = 0, min_rows = 1, min_spans = 1;
};

}  // namespace

struct ktr_tracker {
  int device = 0, nbins = 0, max_spans = 0, capacity = 0, last_grid = 0;
  Params par;
  ksa::track::Key* keys = nullptr;              // device [max_spans]
  int* parent = nullptr;                        // device [max_spans]
  ksa::track::Acc* acc = nullptr;               // device [max_spans]
  int* labels = nullptr;                        // device [max_spans]
  int* block_cnt = nullptr;                     // device [2 * blocks of max_spans]
  int* block_off = nullptr;                     // device [blocks of max_spans]
  long long* counters = nullptr;                // device [4]: tracks_total, components_total, bad_spans, n
  ksa::track::Track* tracks = nullptr;          // device [capacity]
  ksa::track::Span* stage = nullptr;            // device, made by the first ktr_link
  long long stage_spans = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_stream = nullptr;
};

namespace {

// the linking parameters' own rules, shared by ktr_create and ktr_set_params
int check_params(int nbins, int row_gap, int bin_slop, int min_rows, int min_spans, Params* out) {
  if (row_gap < 0 || row_gap > KTR_MAX_ROW_GAP) return fail("row_gap %d outside 0..%d", row_gap, KTR_MAX_ROW_GAP);
  if (bin_slop < 0 || bin_slop > nbins) return fail("bin_slop %d outside 0..nbins = %d", bin_slop, nbins);
  if (min_rows < 1) return fail("min_rows %d must be >= 1", min_rows);
  if (min_spans < 1) return fail("min_spans %d must be >= 1", min_spans);
  out->row_gap = row_gap;
  out->bin_slop = bin_slop;
  out->min_rows = min_rows;
  out->min_spans = min_spans;
  return 0;
}

int blocks_for(long long n) { return (int)std::max<long long>(1, (n + ksa::track::THREADS - 1) / ksa::track::THREADS); }

// the validity rule of the header on host memory: the first index that breaks it, -1 when none does
long long first_bad_span(const ktr_span* s, long long n, int nbins, long long row_end) {
  for (long long i = 0; i < n; ++i) {
    bool bad = s[i].bin_lo < 0 || s[i].bin_lo > s[i].bin_hi || s[i].bin_hi >= nbins || s[i].row < 0 || s[i].row >= row_end;
    if (i > 0)
      bad = bad || !(s[i].row > s[i - 1].row ||
                     (s[i].row == s[i - 1].row && s[i].bin_lo > s[i - 1].bin_lo && s[i].bin_lo > s[i - 1].bin_hi));
    if (bad) return i;
  }
  return -1;
}

// the eight launches of a link over spans_dev[0, n_max); the caller has set the device and n_max >= 1
int launch_link(ktr_tracker* t, const void* spans_dev, long long n_max, const int64_t* n_dev, long long row_end, int32_t* labels_dev) {
  using namespace ksa::track;
  Args a;
  a.spans = static_cast<const Span*>(spans_dev);
  a.n_dev = reinterpret_cast<const long long*>(n_dev);
  a.n_max = n_max;
  a.row_end = row_end;
  a.nbins = t->nbins;
  a.row_gap = t->par.row_gap;
  a.bin_slop = t->par.bin_slop;
  a.min_rows = t->par.min_rows;
  a.min_spans = t->par.min_spans;
  a.capacity = t->capacity;
  a.keys = t->keys;
  a.parent = t->parent;
  a.acc = t->acc;
  a.labels = t->labels;
  a.labels_out = labels_dev;
  a.block_cnt = t->block_cnt;
  a.block_off = t->block_off;
  a.counters = t->counters;
  a.tracks = t->tracks;
  const int grid = blocks_for(n_max);
  t->last_grid = grid;
  HIP_OK(hipMemsetAsync(t->counters, 0, 32, t->stream));
  hipLaunchKernelGGL(validate_kernel, dim3(grid), dim3(THREADS), 0, t->stream, a);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(link_kernel, dim3(grid), dim3(THREADS), 0, t->stream, a);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(flatten_kernel, dim3(grid), dim3(THREADS), 0, t->stream, a);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(reduce_kernel, dim3(grid), dim3(THREADS), 0, t->stream, a);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(mark_kernel, dim3(grid), dim3(THREADS), 0, t->stream, a);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, t->stream, a);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(compact_kernel, dim3(grid), dim3(THREADS), 0, t->stream, a);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(labels_kernel, dim3(grid), dim3(THREADS), 0, t->stream, a);
  HIP_OK(hipGetLastError());
  return 0;
}

void free_all(ktr_tracker* t) {
  if (t->ev_stream) (void)hipEventDestroy(t->ev_stream);
  free_device({t->keys, t->parent, t->acc, t->labels, t->block_cnt, t->block_off, t->counters, t->tracks, t->stage});
  delete t;
}

}  // namespace

extern "C" {

int ktr_abi_version(void) { return KTR_ABI_VERSION; }
const char* ktr_last_error(void) { return g_err.c_str(); }

int ktr_create(int32_t device, int32_t nbins, int32_t max_spans, int32_t row_gap, int32_t bin_slop, int32_t min_rows,
               int32_t min_spans, int32_t capacity, ktr_tracker** out) {
  if (!out) return fail("null out pointer");
  *out = nullptr;
  if (nbins < 1 || nbins > KTR_MAX_NBINS) return fail("nbins %d outside 1..%d", nbins, KTR_MAX_NBINS);
  if (max_spans < 1 || max_spans > KTR_MAX_SPANS) return fail("max_spans %d outside 1..%d", max_spans, KTR_MAX_SPANS);
  Params par;
  if (int rc = check_params(nbins, row_gap, bin_slop, min_rows, min_spans, &par)) return rc;
  if (capacity < 1 || capacity > KTR_MAX_CAPACITY) return fail("track capacity %d outside 1..%d", capacity, KTR_MAX_CAPACITY);
  if (check_device(device)) return 1;

  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(device));
  ktr_tracker* t = new ktr_tracker;
  t->device = device; t->nbins = nbins; t->max_spans = max_spans; t->capacity = capacity; t->par = par;
  int rc = 0;
  do {
    const size_t spans = (size_t)max_spans, blocks = (size_t)blocks_for(max_spans);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&t->keys), spans * sizeof(ksa::track::Key));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&t->parent), spans * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&t->acc), spans * sizeof(ksa::track::Acc));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&t->labels), spans * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&t->block_cnt), blocks * 2 * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&t->block_off), blocks * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&t->counters), 32);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&t->tracks), (size_t)capacity * sizeof(ksa::track::Track));
    if (e != hipSuccess) { rc = fail("hipMalloc of the tracker's device memory failed: %s", hipGetErrorString(e)); break; }
    e = hipMemsetAsync(t->counters, 0, 32, t->stream);
    if (e == hipSuccess) e = hipMemsetAsync(t->tracks, 0, (size_t)capacity * sizeof(ksa::track::Track), t->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
    if (e != hipSuccess) { rc = fail("zeroing the tracker's device memory failed: %s", hipGetErrorString(e)); break; }
  } while (0);
  if (rc) {
    free_all(t);
    return rc;
  }
  *out = t;
  return 0;
}

void ktr_destroy(ktr_tracker* t) {
  if (!t) return;
  DeviceGuard dev_guard;
  (void)hipSetDevice(t->device);
  (void)hipStreamSynchronize(t->stream);
  free_all(t);
}

int ktr_set_stream(ktr_tracker* t, void* hip_stream) {
  if (!t) return fail("null tracker object");
  return hand_over_stream(t->device, &t->stream, &t->ev_stream, hip_stream);
}

int ktr_synchronize(ktr_tracker* t) {
  if (!t) return fail("null tracker object");
  return synchronize_on(t->device, t->stream);
}

int ktr_set_params(ktr_tracker* t, int32_t row_gap, int32_t bin_slop, int32_t min_rows, int32_t min_spans) {
  if (!t) return fail("null tracker object");
  Params par;
  if (int rc = check_params(t->nbins, row_gap, bin_slop, min_rows, min_spans, &par)) return rc;
  t->par = par;                                 // a launch carries its parameters by value: enqueued links keep the old ones
  return 0;
}

int ktr_link_dev(ktr_tracker* t, const void* spans_dev, int64_t n_max, const int64_t* n_dev, int64_t row_end, int32_t* labels_dev) {
  if (!t) return fail("null tracker object");
  if (n_max < 0) return fail("n_max %lld must be >= 0", (long long)n_max);
  if (n_max > t->max_spans) return fail("n_max %lld exceeds max_spans %d", (long long)n_max, t->max_spans);
  if (row_end < 0) return fail("row_end %lld must be >= 0", (long long)row_end);
  if (!spans_dev && n_max > 0) return fail("null spans pointer");
  if (reinterpret_cast<uintptr_t>(spans_dev) & 7) return fail("spans pointer is not 8-byte aligned");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(t->device));
  if (n_max == 0) {                             // nothing to walk: an empty result
    HIP_OK(hipMemsetAsync(t->counters, 0, 32, t->stream));
    return 0;
  }
  return launch_link(t, spans_dev, n_max, n_dev, row_end, labels_dev);
}

int ktr_link(ktr_tracker* t, const void* spans_host, int64_t n, int64_t row_end, int32_t* labels_host) {
  if (!t) return fail("null tracker object");
  if (n < 0) return fail("n %lld must be >= 0", (long long)n);
  if (n > t->max_spans) return fail("n %lld exceeds max_spans %d", (long long)n, t->max_spans);
  if (row_end < 0) return fail("row_end %lld must be >= 0", (long long)row_end);
  if (!spans_host && n > 0) return fail("null spans pointer");
  const long long bad = first_bad_span(static_cast<const ktr_span*>(spans_host), n, t->nbins, row_end);
  if (bad >= 0) {
    const ktr_span* s = static_cast<const ktr_span*>(spans_host) + bad;
    return fail("span %lld (row %lld, bins %d..%d) is not valid: out of range for %d bins and row_end %lld, or not after its "
                "predecessor in strictly ascending (row, bin_lo) order without overlap",
                bad, (long long)s->row, s->bin_lo, s->bin_hi, t->nbins, (long long)row_end);
  }
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(t->device));
  if (n == 0) {
    HIP_OK(hipMemsetAsync(t->counters, 0, 32, t->stream));
    HIP_OK(hipStreamSynchronize(t->stream));
    return 0;
  }
  if (int rc = grow_device(&t->stage, &t->stage_spans, n, t->stream)) return rc;
  HIP_OK(hipMemcpyAsync(t->stage, spans_host, (size_t)n * sizeof(ktr_span), hipMemcpyHostToDevice, t->stream));
  if (int rc = launch_link(t, t->stage, n, nullptr, row_end, nullptr)) return rc;
  if (labels_host) HIP_OK(hipMemcpyAsync(labels_host, t->labels, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
  HIP_OK(hipStreamSynchronize(t->stream));
  return 0;
}

int ktr_read_tracks(ktr_tracker* t, void* records_host, int64_t max_records, int64_t* stored, int64_t* total, int64_t* components,
                    int64_t* bad_spans) {
  if (!t) return fail("null tracker object");
  if (max_records < 0) return fail("max_records %lld must be >= 0", (long long)max_records);
  if (!records_host && !stored && !total && !components && !bad_spans) return fail("null records and count pointers");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(t->device));
  long long c[4] = {0, 0, 0, 0};
  HIP_OK(hipMemcpyAsync(c, t->counters, 32, hipMemcpyDeviceToHost, t->stream));
  HIP_OK(hipStreamSynchronize(t->stream));
  const long long kept = std::min<long long>(c[ksa::track::C_TRACKS], t->capacity);
  const long long n = records_host ? std::min<long long>(kept, max_records) : 0;
  if (n > 0) {
    HIP_OK(hipMemcpyAsync(records_host, t->tracks, (size_t)n * sizeof(ktr_track), hipMemcpyDeviceToHost, t->stream));
    HIP_OK(hipStreamSynchronize(t->stream));
  }
  if (stored) *stored = kept;
  if (total) *total = c[ksa::track::C_TRACKS];
  if (components) *components = c[ksa::track::C_COMPONENTS];
  if (bad_spans) *bad_spans = c[ksa::track::C_BAD];
  return 0;
}

int ktr_read_labels(ktr_tracker* t, int32_t* labels_host, int64_t max_labels, int64_t* n_spans) {
  if (!t) return fail("null tracker object");
  if (max_labels < 0) return fail("max_labels %lld must be >= 0", (long long)max_labels);
  if (!labels_host && !n_spans) return fail("null labels and n_spans pointers");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(t->device));
  long long c[4] = {0, 0, 0, 0};
  HIP_OK(hipMemcpyAsync(c, t->counters, 32, hipMemcpyDeviceToHost, t->stream));
  HIP_OK(hipStreamSynchronize(t->stream));
  const long long n = labels_host ? std::min<long long>(c[ksa::track::C_N], max_labels) : 0;
  if (n > 0) {
    HIP_OK(hipMemcpyAsync(labels_host, t->labels, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
    HIP_OK(hipStreamSynchronize(t->stream));
  }
  if (n_spans) *n_spans = c[ksa::track::C_N];
  return 0;
}

int ktr_tracks_dev(ktr_tracker* t, void** records_dev, int64_t** counters_dev) {
  if (!t) return fail("null tracker object");
  if (!records_dev && !counters_dev) return fail("null records and counters out pointers");
  if (records_dev) *records_dev = t->tracks;
  if (counters_dev) *counters_dev = reinterpret_cast<int64_t*>(t->counters);
  return 0;
}

int ktr_clear(ktr_tracker* t) {
  if (!t) return fail("null tracker object");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(t->device));
  HIP_OK(hipMemsetAsync(t->counters, 0, 32, t->stream));
  return 0;
}

int ktr_kernel_info(ktr_tracker* t, int32_t* threads, int32_t* lds_bytes, int32_t* vgprs, int32_t* grid, int32_t* launches) {
  if (!t) return fail("null tracker object");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(t->device));
  hipFuncAttributes attr;
  HIP_OK(hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(ksa::track::link_kernel)));
  if (threads) *threads = ksa::track::THREADS;
  if (lds_bytes) *lds_bytes = (int32_t)attr.sharedSizeBytes;
  if (vgprs) *vgprs = attr.numRegs;
  if (grid) *grid = t->last_grid ? t->last_grid : blocks_for(t->max_spans);
  if (launches) *launches = ksa::track::LAUNCHES;
  return 0;
}

}  // extern "C"
