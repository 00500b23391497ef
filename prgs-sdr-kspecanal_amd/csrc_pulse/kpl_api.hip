// libksa_pulse: host layer of include/ksa_pulse.h (validation, launch planning, stream state, staging); kernels in
// kpl_kernels.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/ksa_pulse.h"
#include "kpl_kernels.hpp"
#include "../csrc_shared/ksa_host.hpp"

static_assert(sizeof(kpl_pulse) == 8 * ksa::pulse::REC_WORDS, "kpl_pulse and the kernels' record are one layout");
static_assert(KPL_FMT_C64 == ksa::iq::FMT_C64 && KPL_FMT_U8 == ksa::iq::FMT_U8 && KPL_FMT_S8 == ksa::iq::FMT_S8 &&
                  KPL_FMT_S16 == ksa::iq::FMT_S16,
              "the formats of the header are the kernels'");
static_assert(KPL_FLAG_OPEN_END == ksa::pulse::FLAG_OPEN_END, "the flag of the header is the kernels'");

struct kpl_detector {
  int device = 0, fmt = 0, W = 1, min_len = 1, capacity = 0, last_grid = 0, cur = 0;
  bool lost = false;                            // a stream call failed between its launches: kpl_reset starts anew
  bool flushed = false;
  float u8_offset = 127.5f, u8_inv_scale = 1.f / 127.5f, on_power = 1.f, off_power = 1.f;
  long long thr_on = 0, thr_off = 0;
  long long max_in = 0, tiles_cap = 0;
  long long n_in = 0;                           // samples in
  long long* qhist[2] = {nullptr, nullptr};     // device, q of the stream's last W-1 samples and the ones being written
  long long* state = nullptr;                   // device [ST_WORDS]: both totals, the hysteresis state, the open run, the last sample
  long long* S = nullptr;                       // device work [max_in]
  long long* events = nullptr;                  // device [capacity] records
  int* tile_ints = nullptr;                     // device [4][tiles_cap]: summary, state_in, info, cnt
  long long* tile_lls = nullptr;                // device [2][tiles_cap]: act, off
  ksa::pulse::Rec* tile_recs = nullptr;         // device [2][tiles_cap]: head, tail
  char* stage = nullptr;                        // kpl_process: the call's input
  long long stage_bytes = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_stream = nullptr;
};

namespace {

using ksa::pulse::ST_WORDS;
using ksa::pulse::THREADS;
using ksa::pulse::TILE;

// an empty stream: totals zero, inactive, no open run, the last sample (0, 0)
const long long FRESH_STATE[ST_WORDS] = {0, 0, 0, 0, 0, -1, 0x7fffffffffffffffll, 0, 0, 0};

int in_bytes(const kpl_detector* h) { return iq_sample_bytes(h->fmt); }
size_t events_bytes(const kpl_detector* h) { return (size_t)h->capacity * sizeof(kpl_pulse); }
size_t hist_bytes(const kpl_detector* h) { return (size_t)std::max(h->W - 1, 1) * sizeof(long long); }
int env_lds_bytes(const kpl_detector* h) { return (TILE + h->W) * (int)sizeof(long long); }

void free_tiles(kpl_detector* h) {
  free_device({h->tile_ints, h->tile_lls, h->tile_recs});
  h->tile_ints = nullptr;
  h->tile_lls = nullptr;
  h->tile_recs = nullptr;
  h->tiles_cap = 0;
}

void free_all(kpl_detector* h) {
  if (h->ev_stream) (void)hipEventDestroy(h->ev_stream);
  free_tiles(h);
  free_device({h->qhist[0], h->qhist[1], h->state, h->S, h->events, h->stage});
  delete h;
}

// the per-tile memory holds `need` tiles afterwards; a larger one replaces it once the stream's work on the old one is done
int ensure_tiles(kpl_detector* h, long long need) {
  if (h->tiles_cap >= need) return 0;
  HIP_OK(hipStreamSynchronize(h->stream));
  free_tiles(h);
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->tile_ints), (size_t)need * 4 * sizeof(int));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->tile_lls), (size_t)need * 2 * sizeof(long long));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->tile_recs), (size_t)need * 2 * sizeof(ksa::pulse::Rec));
  if (e != hipSuccess) {
    free_tiles(h);
    return fail("hipMalloc of the detector's per-tile memory for %lld tiles failed: %s", need, hipGetErrorString(e));
  }
  h->tiles_cap = need;
  return 0;
}

int check_params(float on_power, float off_power, int W, long long* thr_on, long long* thr_off) {
  if (!(std::isfinite(on_power) && on_power > 0.f && on_power <= 4.f))
    return fail("on_power %g is not a finite value in (0, 4]", (double)on_power);
  if (!(std::isfinite(off_power) && off_power > 0.f && off_power <= on_power))
    return fail("off_power %g is not a finite value in (0, on_power = %g]", (double)off_power, (double)on_power);
  const long long on = std::llrint((double)on_power * 1073741824.0 * W), off = std::llrint((double)off_power * 1073741824.0 * W);
  if (off < 1) return fail("off_power %g gives thr_off %lld below 1 at W %d", (double)off_power, off, W);
  *thr_on = on;
  *thr_off = off;
  return 0;
}

ksa::pulse::Args base_args(const kpl_detector* h) {
  ksa::pulse::Args a{};
  const long long n = h->tiles_cap;
  a.state = h->state;
  a.S = h->S;
  a.events = h->events;
  a.summary = h->tile_ints;
  a.state_in = h->tile_ints + n;
  a.info = h->tile_ints + 2 * n;
  a.cnt = h->tile_ints + 3 * n;
  a.act = h->tile_lls;
  a.off = h->tile_lls + n;
  a.head = h->tile_recs;
  a.tail = h->tile_recs + n;
  a.thr_on = h->thr_on;
  a.thr_off = h->thr_off;
  a.fmt = h->fmt;
  a.u8_offset = h->u8_offset;
  a.u8_inv_scale = h->u8_inv_scale;
  a.W = h->W;
  a.min_len = h->min_len;
  a.capacity = h->capacity;
  return a;
}

template <int FMT> int launch_fmt(kpl_detector* h, const ksa::pulse::Args& a, long long nblocks, bool* launched) {
  using namespace ksa::pulse;
  const dim3 grid((unsigned)a.ntiles), wg(THREADS);
  hipLaunchKernelGGL(env_kernel<FMT>, grid, wg, (size_t)env_lds_bytes(h), h->stream, a);
  HIP_OK(hipGetLastError());
  *launched = true;
  h->last_grid = (int)a.ntiles;
  hipLaunchKernelGGL(state_kernel, dim3((unsigned)nblocks), wg, 0, h->stream, a);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL((runs_kernel<FMT, false>), grid, wg, 0, h->stream, a);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(stitch_kernel, dim3(1), wg, 0, h->stream, a);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL((runs_kernel<FMT, true>), grid, wg, 0, h->stream, a);
  HIP_OK(hipGetLastError());
  if (a.stream) {
    hipLaunchKernelGGL(hist_kernel<FMT>, dim3((unsigned)ceil_div(std::max(a.W - 1, 1), THREADS)), wg, 0, h->stream, a, h->qhist[h->cur ^ 1]);
    HIP_OK(hipGetLastError());
  }
  return 0;
}

// nblocks blocks of a.len > 0 samples: envelope, states, runs, stitch, records and, in the stream form, the history
int launch_all(kpl_detector* h, ksa::pulse::Args& a, long long nblocks, bool* launched) {
  a.tiles = (int)ceil_div(a.len, TILE);
  a.ntiles = a.tiles * nblocks;
  switch (h->fmt) {
    case KPL_FMT_C64: return launch_fmt<KPL_FMT_C64>(h, a, nblocks, launched);
    case KPL_FMT_U8: return launch_fmt<KPL_FMT_U8>(h, a, nblocks, launched);
    case KPL_FMT_S8: return launch_fmt<KPL_FMT_S8>(h, a, nblocks, launched);
    default: return launch_fmt<KPL_FMT_S16>(h, a, nblocks, launched);
  }
}

// The next n > 0 samples of the stream at in (device-visible).
int stream_call(kpl_detector* h, const void* in, long long n, long long* env) {
  ksa::pulse::Args a = base_args(h);
  a.in = in;
  a.qhist = h->qhist[h->cur];
  a.env = env;
  a.pos_base = h->n_in;
  a.len = (int)n;
  a.stream = 1;
  bool launched = false;
  if (int rc = launch_all(h, a, 1, &launched)) {              // outputs or records may be written, the carried state half moved
    h->lost = h->lost || launched;
    return rc;
  }
  h->cur ^= 1;
  h->n_in += n;
  return 0;
}

int check_stream_args(kpl_detector* h, const void* in, int64_t n_in) {
  if (!h) return fail("null detector object");
  if (n_in < 0) return fail("n_in %lld must be >= 0", (long long)n_in);
  if (n_in > h->max_in) return fail("n_in %lld exceeds max_in %lld", (long long)n_in, h->max_in);
  if (n_in > 0 && !in) return fail("null input pointer");
  if (int rc = check_iq_aligned(in, in_bytes(h))) return rc;
  if (h->flushed) return fail("the stream was flushed; kpl_reset starts a new stream");
  if (h->lost) return fail("the stream state was lost when an earlier call failed after its first launch; kpl_reset starts a new stream");
  if (n_in > KPL_MAX_POSITION - h->n_in)
    return fail("n_in %lld would take the stream from %lld samples past 2^52", (long long)n_in, h->n_in);
  return 0;
}

}  // namespace

extern "C" {

int kpl_abi_version(void) { return KPL_ABI_VERSION; }
const char* kpl_last_error(void) { return g_err.c_str(); }

int kpl_create(int32_t device, int32_t fmt, float u8_offset, float u8_scale, int32_t W, float on_power, float off_power,
               int32_t min_len, int32_t capacity, int64_t max_in, kpl_detector** out) {
  if (!out) return fail("null out pointer");
  *out = nullptr;
  if (check_iq_format(fmt)) return 1;
  if (W < 1 || W > KPL_MAX_W) return fail("W %d outside 1..%d", W, KPL_MAX_W);
  long long thr_on = 0, thr_off = 0;
  if (int rc = check_params(on_power, off_power, W, &thr_on, &thr_off)) return rc;
  if (min_len < 1 || min_len > KPL_MAX_MIN_LEN) return fail("min_len %d outside 1..%d", min_len, KPL_MAX_MIN_LEN);
  if (capacity < 1 || capacity > KPL_MAX_CAPACITY) return fail("pulse capacity %d outside 1..%d", capacity, KPL_MAX_CAPACITY);
  if (max_in < 1 || max_in > KPL_MAX_IN) return fail("max_in %lld outside 1..%d", (long long)max_in, KPL_MAX_IN);
  if (check_u8_scaling(fmt, u8_offset, u8_scale)) return 1;
  if (check_device(device)) return 1;

  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(device));
  kpl_detector* h = new kpl_detector;
  h->device = device; h->fmt = fmt; h->W = W; h->min_len = min_len; h->capacity = capacity; h->max_in = max_in;
  h->on_power = on_power; h->off_power = off_power; h->thr_on = thr_on; h->thr_off = thr_off;
  if (fmt == KPL_FMT_U8) { h->u8_offset = u8_offset; h->u8_inv_scale = 1.0f / u8_scale; }
  int rc = 0;
  do {
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->qhist[0]), hist_bytes(h));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->qhist[1]), hist_bytes(h));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->state), sizeof FRESH_STATE);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->S), (size_t)max_in * sizeof(long long));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->events), events_bytes(h));
    if (e != hipSuccess) { rc = fail("hipMalloc of the detector's device memory failed: %s", hipGetErrorString(e)); break; }
    if ((rc = ensure_tiles(h, ceil_div(max_in, TILE) + 1))) break;
    e = hipMemsetAsync(h->events, 0, events_bytes(h), h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->qhist[0], 0, hist_bytes(h), h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h->state, FRESH_STATE, sizeof FRESH_STATE, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { rc = fail("filling the detector's device memory failed: %s", hipGetErrorString(e)); break; }
  } while (0);
  if (rc) {
    free_all(h);
    return rc;
  }
  *out = h;
  return 0;
}

void kpl_destroy(kpl_detector* h) {
  if (!h) return;
  DeviceGuard dev_guard;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  free_all(h);
}

int kpl_set_stream(kpl_detector* h, void* hip_stream) {
  if (!h) return fail("null detector object");
  return hand_over_stream(h->device, &h->stream, &h->ev_stream, hip_stream);
}

int kpl_synchronize(kpl_detector* h) {
  if (!h) return fail("null detector object");
  return synchronize_on(h->device, h->stream);
}

int kpl_process_dev(kpl_detector* h, const void* iq_dev, int64_t n_in, int64_t* env_dev) {
  if (int rc = check_stream_args(h, iq_dev, n_in)) return rc;
  if (n_in == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  return stream_call(h, iq_dev, n_in, reinterpret_cast<long long*>(env_dev));
}

int kpl_process(kpl_detector* h, const void* iq_host, int64_t n_in, int64_t* env_host) {
  if (int rc = check_stream_args(h, iq_host, n_in)) return rc;
  if (n_in == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  const long long bytes = (long long)n_in * in_bytes(h);
  if (int rc = grow_device(&h->stage, &h->stage_bytes, bytes, h->stream)) return rc;
  HIP_OK(hipMemcpyAsync(h->stage, iq_host, (size_t)bytes, hipMemcpyHostToDevice, h->stream));
  if (int rc = stream_call(h, h->stage, n_in, nullptr)) return rc;
  if (env_host) HIP_OK(hipMemcpyAsync(env_host, h->S, (size_t)n_in * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

int kpl_flush(kpl_detector* h) {
  if (!h) return fail("null detector object");
  if (h->flushed) return fail("the stream was flushed; kpl_reset starts a new stream");
  if (h->lost) return fail("the stream state was lost when an earlier call failed after its first launch; kpl_reset starts a new stream");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  ksa::pulse::Args a = base_args(h);
  a.pos_base = h->n_in;
  a.stream = 1;
  a.final = 1;
  hipLaunchKernelGGL(ksa::pulse::stitch_kernel, dim3(1), dim3(THREADS), 0, h->stream, a);
  HIP_OK(hipGetLastError());
  h->flushed = true;
  return 0;
}

int kpl_blocks_dev(kpl_detector* h, const void* iq_dev, int64_t block_stride, int64_t nblocks, int64_t block_len, int64_t* env_dev,
                   int64_t out_stride) {
  if (!h) return fail("null detector object");
  if (nblocks < 0) return fail("nblocks %lld must be >= 0", (long long)nblocks);
  if (block_stride < 0) return fail("block_stride %lld must be >= 0", (long long)block_stride);
  if (block_len < 0) return fail("block_len %lld must be >= 0", (long long)block_len);
  if (block_len > h->max_in || (block_len > 0 && nblocks > h->max_in / block_len))
    return fail("%lld blocks of %lld samples exceed max_in %lld", (long long)nblocks, (long long)block_len, h->max_in);
  if (nblocks > 0 && block_len > 0 && !iq_dev) return fail("null input pointer");
  if (int rc = check_iq_aligned(iq_dev, in_bytes(h))) return rc;
  if (env_dev && out_stride < block_len)
    return fail("out_stride %lld is shorter than the %lld samples of a block", (long long)out_stride, (long long)block_len);
  if (nblocks == 0 || block_len == 0) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  if (int rc = ensure_tiles(h, nblocks * ceil_div(block_len, TILE))) return rc;
  ksa::pulse::Args a = base_args(h);
  a.in = iq_dev;
  a.block_stride = block_stride;
  a.env = reinterpret_cast<long long*>(env_dev);
  a.out_stride = out_stride;
  a.len = (int)block_len;
  a.final = 1;
  bool launched = false;
  return launch_all(h, a, nblocks, &launched);
}

int kpl_set_params(kpl_detector* h, float on_power, float off_power) {
  if (!h) return fail("null detector object");
  long long thr_on = 0, thr_off = 0;
  if (int rc = check_params(on_power, off_power, h->W, &thr_on, &thr_off)) return rc;
  h->on_power = on_power;                       // a launch carries its parameters by value: enqueued work keeps the old ones
  h->off_power = off_power;
  h->thr_on = thr_on;
  h->thr_off = thr_off;
  return 0;
}

int kpl_thresholds(kpl_detector* h, int64_t* thr_on, int64_t* thr_off) {
  if (!h) return fail("null detector object");
  if (thr_on) *thr_on = h->thr_on;
  if (thr_off) *thr_off = h->thr_off;
  return 0;
}

int kpl_reset(kpl_detector* h) {
  if (!h) return fail("null detector object");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  HIP_OK(hipMemsetAsync(h->events, 0, events_bytes(h), h->stream));
  HIP_OK(hipMemsetAsync(h->qhist[h->cur], 0, hist_bytes(h), h->stream));
  HIP_OK(hipMemcpyAsync(h->state, FRESH_STATE, sizeof FRESH_STATE, hipMemcpyHostToDevice, h->stream));
  h->n_in = 0;
  h->lost = false;
  h->flushed = false;
  return 0;
}

int kpl_state(kpl_detector* h, int64_t* samples_in, int32_t* open, int64_t* open_start) {
  if (!h) return fail("null detector object");
  if (open || open_start) {
    DeviceGuard dev_guard;
    HIP_OK(hipSetDevice(h->device));
    long long st[2] = {0, 0};                   // the state and the open run's length
    HIP_OK(hipMemcpyAsync(st, h->state + ksa::pulse::ST_STATE, sizeof st, hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
    if (open) *open = st[0] ? 1 : 0;
    if (open_start) *open_start = st[0] ? h->n_in - st[1] : -1;
  }
  if (samples_in) *samples_in = h->n_in;
  return 0;
}

int kpl_read_events(kpl_detector* h, void* records_host, int64_t max_records, int64_t* stored, int64_t* total, int64_t* active) {
  if (!h) return fail("null detector object");
  if (max_records < 0) return fail("max_records %lld must be >= 0", (long long)max_records);
  if (!records_host && !stored && !total && !active) return fail("null records, stored, total and active pointers");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  long long all[2] = {0, 0};
  HIP_OK(hipMemcpyAsync(all, h->state, sizeof all, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  const long long kept = std::min<long long>(all[0], h->capacity);
  const long long n = records_host ? std::min<long long>(kept, max_records) : 0;
  if (n > 0) {
    HIP_OK(hipMemcpyAsync(records_host, h->events, (size_t)n * sizeof(kpl_pulse), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
  }
  if (stored) *stored = kept;
  if (total) *total = all[0];
  if (active) *active = all[1];
  return 0;
}

int kpl_events_dev(kpl_detector* h, void** records_dev, int64_t** totals_dev) {
  if (!h) return fail("null detector object");
  if (!records_dev && !totals_dev) return fail("null records and totals out pointers");
  if (records_dev) *records_dev = h->events;
  if (totals_dev) *totals_dev = reinterpret_cast<int64_t*>(h->state);
  return 0;
}

int kpl_clear_events(kpl_detector* h) {
  if (!h) return fail("null detector object");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  HIP_OK(hipMemsetAsync(h->events, 0, events_bytes(h), h->stream));
  HIP_OK(hipMemsetAsync(h->state, 0, 2 * sizeof(long long), h->stream));
  return 0;
}

int kpl_kernel_info(kpl_detector* h, int32_t* threads, int32_t* lds_bytes, int32_t* vgprs, int32_t* grid, int32_t* tile) {
  if (!h) return fail("null detector object");
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(h->device));
  using namespace ksa::pulse;
  const void* fn = h->fmt == KPL_FMT_C64  ? reinterpret_cast<const void*>(env_kernel<KPL_FMT_C64>)
                   : h->fmt == KPL_FMT_U8 ? reinterpret_cast<const void*>(env_kernel<KPL_FMT_U8>)
                   : h->fmt == KPL_FMT_S8 ? reinterpret_cast<const void*>(env_kernel<KPL_FMT_S8>)
                                          : reinterpret_cast<const void*>(env_kernel<KPL_FMT_S16>);
  hipFuncAttributes attr;
  HIP_OK(hipFuncGetAttributes(&attr, fn));
  if (threads) *threads = THREADS;
  if (lds_bytes) *lds_bytes = (int32_t)attr.sharedSizeBytes + env_lds_bytes(h);
  if (vgprs) *vgprs = attr.numRegs;
  if (grid) *grid = h->last_grid ? h->last_grid : (int32_t)ceil_div(h->max_in, TILE);
  if (tile) *tile = TILE;
  return 0;
}

}  // extern "C"
