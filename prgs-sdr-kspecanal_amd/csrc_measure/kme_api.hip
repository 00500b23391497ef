// libksa_measure: host layer of include/ksa_measure.h (validation, launch planning, staging); the kernel is in kme_kernels.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/ksa_measure.h"
#include "kme_kernels.hpp"
#include "../csrc_shared/ksa_host.hpp"

static_assert(sizeof(kme_result) == sizeof(ksa::measure::Result), "kme_result and the kernel's record are one layout");
static_assert(offsetof(kme_result, power) == offsetof(ksa::measure::Result, power) &&
                  offsetof(kme_result, peak_bin) == offsetof(ksa::measure::Result, peak_bin) &&
                  offsetof(kme_result, power_db) == offsetof(ksa::measure::Result, power_db),
              "kme_result and the kernel's record are one layout");
static_assert(KME_WAVE_MAX_BINS == ksa::measure::WAVE_MAX_BINS && KME_FLAG_MEASURED == ksa::measure::FLAG_MEASURED &&
                  KME_FLAG_CLIPPED == ksa::measure::FLAG_CLIPPED && KME_FLAG_INVALID == ksa::measure::FLAG_INVALID,
              "the constants of the header are the kernel's");
static_assert(sizeof(kme_span) == 16, "what a span record begins with");

namespace {

constexpr long long STAGE_BYTES = 64ll << 20;           // host rows cross in pieces of at most this size
constexpr int WG_PER_CU = 8;                            // 2048 threads of a CU

struct Params {
  float beta = 0.f, xdb = 0.f;
  int margin = 0;
};

}  // namespace

struct kme_meter {
  int device = 0, nbins = 0, capacity = 0, cus = 1, nb = 0;
  int last_grid = 0, last_vec = -1, last_form = 0;
  bool narrow = false, wide = false;            // the bands hold a window for the wave form / for the workgroup form
  Params par;
  ksa::measure::Result* results = nullptr;      // device [capacity]
  int* bands = nullptr;                         // device [KME_MAX_BANDS][2]
  std::vector<int32_t> bands_host;
  float* stage = nullptr;
  long long stage_floats = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_stream = nullptr;
};

namespace {

// the measurement parameters' own rules, shared by kme_create and kme_set_params
int check_params(float occupied, float xdb, int margin, Params* out) {
  if (!(occupied >= 0.5f && occupied < 1.0f)) return fail("occupied %g is not a share in 0.5 <= occupied < 1", (double)occupied);
  if (!std::isfinite(xdb) || xdb < 0.0f || xdb > 100.0f) return fail("xdb %g is not a finite value in 0..100", (double)xdb);
  if (margin < 0 || margin > KME_MAX_MARGIN) return fail("margin %d outside 0..%d", margin, KME_MAX_MARGIN);
  out->beta = occupied;
  out->xdb = xdb;
  out->margin = margin;
  return 0;
}

// what every measuring call checks alike about its rows
int check_rows(const kme_meter* m, const float* rows, long long row_stride, long long nrows, long long row_base) {
  if (!rows) return fail("null rows pointer");
  if (nrows < 0) return fail("nrows %lld must be >= 0", nrows);
  if (row_stride < m->nbins) return fail("row_stride %lld is shorter than a row of %d bins", row_stride, m->nbins);
  if (reinterpret_cast<uintptr_t>(rows) & 3) return fail("rows pointer is not 4-byte aligned");
  if (row_base < 0) return fail("row base %lld must be >= 0", row_base);
  return 0;
}

int check_spans(const void* spans, long long span_stride, const int64_t* total, long long span_capacity, long long first) {
  if (!spans) return fail("null spans pointer");
  if (!total) return fail("null span total pointer");
  if (span_stride < 16 || span_stride % 8) return fail("span stride %lld must be >= 16 bytes and a multiple of 8", span_stride);
  if (span_capacity < 0) return fail("span_capacity %lld must be >= 0", span_capacity);
  if (first < 0) return fail("first %lld must be >= 0", first);
  return 0;
}

int check_slots(const kme_meter* m, long long nrows, long long first_slot) {
  if (first_slot < 0) return fail("first_slot %lld must be >= 0", first_slot);
  if (first_slot > m->capacity || (m->nb > 0 && nrows > (m->capacity - first_slot) / m->nb))
    return fail("result slots %lld .. %lld + %lld rows x %d bands pass the capacity %d", first_slot, first_slot, nrows, m->nb,
                m->capacity);
  return 0;
}

bool vec_for(const kme_meter* m, const float* rows_dev, long long row_stride) {
  return m->nbins % 4 == 0 && (reinterpret_cast<uintptr_t>(rows_dev) & 15) == 0 && row_stride % 4 == 0;
}

const void* kernel_fn(bool wg, bool vec) {
  using namespace ksa::measure;
  if (wg) return vec ? reinterpret_cast<const void*>(measure_kernel<true, true>) : reinterpret_cast<const void*>(measure_kernel<true, false>);
  return vec ? reinterpret_cast<const void*>(measure_kernel<false, true>) : reinterpret_cast<const void*>(measure_kernel<false, false>);
}

// workgroups for at most `tasks` tasks: never more than there are tasks, never more than the device holds at once
int grid_for(const kme_meter* m, long long tasks, bool wg) {
  const long long need = wg ? tasks : (tasks + ksa::measure::WAVES - 1) / ksa::measure::WAVES;
  return (int)std::max<long long>(1, std::min<long long>(need, (long long)m->cus * WG_PER_CU));
}

// one launch of one form over the whole task list; the tasks of the other form are passed over on the device
int launch_form(kme_meter* m, const ksa::measure::Args& a, long long tasks, bool wg, bool vec) {
  using namespace ksa::measure;
  const int grid = grid_for(m, tasks, wg);
  if (wg) {
    if (vec) hipLaunchKernelGGL((measure_kernel<true, true>), dim3(grid), dim3(THREADS), 0, m->stream, a);
    else hipLaunchKernelGGL((measure_kernel<true, false>), dim3(grid), dim3(THREADS), 0, m->stream, a);
  } else {
    if (vec) hipLaunchKernelGGL((measure_kernel<false, true>), dim3(grid), dim3(THREADS), 0, m->stream, a);
    else hipLaunchKernelGGL((measure_kernel<false, false>), dim3(grid), dim3(THREADS), 0, m->stream, a);
  }
  HIP_OK(hipGetLastError());
  m->last_grid = grid;
  m->last_vec = vec ? 1 : 0;
  m->last_form = wg ? 1 : 0;
  return 0;
}

ksa::measure::Args base_args(const kme_meter* m, const float* rows_dev, long long row_stride, long long nrows, long long row_base) {
  ksa::measure::Args a = {};
  a.rows = rows_dev;
  a.row_stride = row_stride;
  a.nrows = nrows;
  a.row_base = row_base;
  a.results = m->results;
  a.capacity = m->capacity;
  a.nbins = m->nbins;
  a.margin = m->par.margin;
  a.beta = m->par.beta;
  a.xdb = m->par.xdb;
  return a;
}

// the widths of the spans are known on the device only: both forms run
int launch_spans(kme_meter* m, const float* rows_dev, long long row_stride, long long nrows, long long row_base,
                 const void* spans_dev, long long span_stride, const int64_t* total_dev, long long span_capacity, long long first) {
  const long long tasks = std::min<long long>(span_capacity, m->capacity) - first;      // at most; the device reads the count
  if (nrows == 0 || tasks <= 0) return 0;
  ksa::measure::Args a = base_args(m, rows_dev, row_stride, nrows, row_base);
  a.spans = static_cast<const unsigned char*>(spans_dev);
  a.span_stride = span_stride;
  a.total = reinterpret_cast<const long long*>(total_dev);
  a.span_capacity = span_capacity;
  a.first = first;
  const bool vec = vec_for(m, rows_dev, row_stride);
  if (int rc = launch_form(m, a, tasks, false, vec)) return rc;
  return launch_form(m, a, tasks, true, vec);
}

int launch_bands(kme_meter* m, const float* rows_dev, long long row_stride, long long nrows, long long row_base,
                 long long first_slot) {
  const long long tasks = nrows * m->nb;
  if (tasks == 0) return 0;
  ksa::measure::Args a = base_args(m, rows_dev, row_stride, nrows, row_base);
  a.bands = m->bands;
  a.nb = m->nb;
  a.first_slot = first_slot;
  const bool vec = vec_for(m, rows_dev, row_stride);
  if (m->narrow)
    if (int rc = launch_form(m, a, tasks, false, vec)) return rc;
  if (m->wide)
    if (int rc = launch_form(m, a, tasks, true, vec)) return rc;
  return 0;
}

// rows of host memory in pieces through the staging buffer: fn(rows_dev, n, row_base of the piece) per piece, then one wait
template <class F> int staged(kme_meter* m, const float* rows_host, long long nrows, long long row_base, F fn) {
  const long long piece = std::max<long long>(1, STAGE_BYTES / ((long long)m->nbins * 4));
  if (int rc = grow_device(&m->stage, &m->stage_floats, std::min(piece, nrows) * m->nbins, m->stream)) return rc;
  // the pieces queue one behind the other on the object's stream, so one staging buffer serves them all
  for (long long done = 0; done < nrows;) {
    const long long n = std::min(piece, nrows - done);
    HIP_OK(hipMemcpyAsync(m->stage, rows_host + done * m->nbins, (size_t)n * m->nbins * 4, hipMemcpyHostToDevice, m->stream));
    if (int rc = fn(m->stage, n, row_base + done)) return rc;
    done += n;
  }
  HIP_OK(hipStreamSynchronize(m->stream));
  return 0;
}

void free_all(kme_meter* m) {
  if (m->ev_stream) (void)hipEventDestroy(m->ev_stream);
  free_device({m->results, m->bands, m->stage});
  delete m;
}

}  // namespace

extern "C" {

int kme_abi_version(void) { return KME_ABI_VERSION; }
const char* kme_last_error(void) { return g_err.c_str(); }

int kme_create(int32_t device, int32_t nbins, int32_t capacity, float occupied, float xdb, int32_t margin, kme_meter** out) {
  if (!out) return fail("null out pointer");
  *out = nullptr;
  if (nbins < 1 || nbins > KME_MAX_NBINS) return fail("nbins %d outside 1..%d", nbins, KME_MAX_NBINS);
  if (capacity < 1 || capacity > KME_MAX_CAPACITY) return fail("result capacity %d outside 1..%d", capacity, KME_MAX_CAPACITY);
  Params par;
  if (int rc = check_params(occupied, xdb, margin, &par)) return rc;
  if (check_device(device)) return 1;

  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(device));
  kme_meter* m = new kme_meter;
  m->device = device; m->nbins = nbins; m->capacity = capacity; m->par = par;
  int rc = 0;
  do {
    if ((rc = cu_count(device, &m->cus))) break;
    const size_t bytes = (size_t)capacity * sizeof(ksa::measure::Result);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&m->results), bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&m->bands), (size_t)KME_MAX_BANDS * 2 * sizeof(int));
    if (e != hipSuccess) { rc = fail("hipMalloc of the meter object's device memory failed: %s", hipGetErrorString(e)); break; }
    e = hipMemsetAsync(m->results, 0, bytes, m->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
    if (e != hipSuccess) { rc = fail("zeroing the meter object's device memory failed: %s", hipGetErrorString(e)); break; }
  } while (0);
  if (rc) {
    free_all(m);
    return rc;
  }
  *out = m;
  return 0;
}

void kme_destroy(kme_meter* m) {
  if (!m) return;
  DeviceGuard dev_guard;
  (void)hipSetDevice(m->device);
  (void)hipStreamSynchronize(m->stream);
  free_all(m);
}

int kme_set_stream(kme_meter* m, void* hip_stream) {
  if (!m) return fail("null meter object");
  return hand_over_stream(m->device, &m->stream, &m->ev_stream, hip_stream);
}

int kme_synchronize(kme_meter* m) {
  if (!m) return fail("null meter object");
  return synchronize_on(m->device, m->stream);
}

int kme_set_params(kme_meter* m, float occupied, float xdb, int32_t margin) {
  if (!m) return fail("null meter object");
  Params par;
  if (int rc = check_params(occupied, xdb, margin, &par)) return rc;
  m->par = par;                                 // a launch carries its parameters by value: enqueued work keeps the old ones
  return 0;
}

int kme_measure_spans_dev(kme_meter* m, const float* rows_dev, int64_t row_stride, int64_t nrows, int64_t row_base,
                          const void* spans_dev, int64_t span_stride_bytes, const int64_t* total_dev, int64_t span_capacity,
                          int64_t first) {
  if (!m) return fail("null meter object");
  if (int rc = check_rows(m, rows_dev, row_stride, nrows, row_base)) return rc;
  if (int rc = check_spans(spans_dev, span_stride_bytes, total_dev, span_capacity, first)) return rc;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(m->device));
  return launch_spans(m, rows_dev, row_stride, nrows, row_base, spans_dev, span_stride_bytes, total_dev, span_capacity, first);
}

int kme_measure_spans(kme_meter* m, const float* rows_host, int64_t nrows, int64_t row_base, const void* spans_dev,
                      int64_t span_stride_bytes, const int64_t* total_dev, int64_t span_capacity, int64_t first) {
  if (!m) return fail("null meter object");
  if (int rc = check_rows(m, rows_host, m->nbins, nrows, row_base)) return rc;
  if (int rc = check_spans(spans_dev, span_stride_bytes, total_dev, span_capacity, first)) return rc;
  if (nrows == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(m->device));
  return staged(m, rows_host, nrows, row_base, [&](const float* rows_dev, long long n, long long base) {
    return launch_spans(m, rows_dev, m->nbins, n, base, spans_dev, span_stride_bytes, total_dev, span_capacity, first);
  });
}

int kme_set_bands(kme_meter* m, const int32_t* bands_host, int32_t nb) {
  if (!m) return fail("null meter object");
  if (nb < 0 || nb > KME_MAX_BANDS) return fail("nb %d outside 0..%d", nb, KME_MAX_BANDS);
  if (nb > 0 && !bands_host) return fail("null bands pointer");
  bool narrow = false, wide = false;
  for (int j = 0; j < nb; ++j) {
    const int lo = bands_host[2 * j], hi = bands_host[2 * j + 1];
    if (lo < 0 || hi >= m->nbins || lo > hi) return fail("band %d [%d, %d] is not inside the %d bins of a row", j, lo, hi, m->nbins);
    (hi - lo + 1 > KME_WAVE_MAX_BINS ? wide : narrow) = true;
  }
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(m->device));
  std::vector<int32_t> copy(bands_host, bands_host + 2 * (size_t)nb);
  if (nb > 0) HIP_OK(hipMemcpyAsync(m->bands, copy.data(), copy.size() * sizeof(int32_t), hipMemcpyHostToDevice, m->stream));
  HIP_OK(hipStreamSynchronize(m->stream));
  m->bands_host.swap(copy);
  m->nb = nb;
  m->narrow = narrow;
  m->wide = wide;
  return 0;
}

int kme_measure_bands_dev(kme_meter* m, const float* rows_dev, int64_t row_stride, int64_t nrows, int64_t row_base,
                          int64_t first_slot) {
  if (!m) return fail("null meter object");
  if (int rc = check_rows(m, rows_dev, row_stride, nrows, row_base)) return rc;
  if (int rc = check_slots(m, nrows, first_slot)) return rc;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(m->device));
  return launch_bands(m, rows_dev, row_stride, nrows, row_base, first_slot);
}

int kme_measure_bands(kme_meter* m, const float* rows_host, int64_t nrows, int64_t row_base, int64_t first_slot) {
  if (!m) return fail("null meter object");
  if (int rc = check_rows(m, rows_host, m->nbins, nrows, row_base)) return rc;
  if (int rc = check_slots(m, nrows, first_slot)) return rc;
  if (nrows == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(m->device));
  return staged(m, rows_host, nrows, row_base, [&](const float* rows_dev, long long n, long long base) {
    return launch_bands(m, rows_dev, m->nbins, n, base, first_slot + (base - row_base) * m->nb);
  });
}

int kme_read_results(kme_meter* m, void* out_host, int64_t first, int64_t count) {
  if (!m) return fail("null meter object");
  if (first < 0) return fail("first %lld must be >= 0", (long long)first);
  if (count < 0) return fail("count %lld must be >= 0", (long long)count);
  if (first > m->capacity || count > m->capacity - first)
    return fail("results %lld .. %lld pass the capacity %d", (long long)first, (long long)(first + count), m->capacity);
  if (count > 0 && !out_host) return fail("null results pointer");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(m->device));
  if (count > 0)
    HIP_OK(hipMemcpyAsync(out_host, m->results + first, (size_t)count * sizeof(kme_result), hipMemcpyDeviceToHost, m->stream));
  HIP_OK(hipStreamSynchronize(m->stream));
  return 0;
}

int kme_results_dev(kme_meter* m, void** results_dev) {
  if (!m) return fail("null meter object");
  if (!results_dev) return fail("null out pointer");
  *results_dev = m->results;
  return 0;
}

int kme_reset(kme_meter* m) {
  if (!m) return fail("null meter object");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(m->device));
  HIP_OK(hipMemsetAsync(m->results, 0, (size_t)m->capacity * sizeof(ksa::measure::Result), m->stream));
  return 0;
}

int kme_kernel_info(kme_meter* m, int32_t* threads, int32_t* lds_bytes, int32_t* vgprs, int32_t* grid, int32_t* vec,
                    int32_t* form) {
  if (!m) return fail("null meter object");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(m->device));
  const bool v = m->last_vec >= 0 ? m->last_vec == 1 : m->nbins % 4 == 0;
  hipFuncAttributes attr;
  HIP_OK(hipFuncGetAttributes(&attr, kernel_fn(m->last_form == 1, v)));
  if (threads) *threads = ksa::measure::THREADS;
  if (lds_bytes) *lds_bytes = (int32_t)attr.sharedSizeBytes;
  if (vgprs) *vgprs = attr.numRegs;
  if (grid) *grid = m->last_grid ? m->last_grid : grid_for(m, 1ll << 40, false);
  if (vec) *vec = v ? 1 : 0;
  if (form) *form = m->last_form;
  return 0;
}

}  // extern "C"
