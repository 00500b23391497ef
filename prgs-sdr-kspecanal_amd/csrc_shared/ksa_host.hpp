// Host layer that the companion libraries share: the error string, the device guard, the create-time checks and the stream,
// device-count and buffer steps that every k??_api.hip used to carry as its own copy.
// csrc_shared/ is a sibling of csrc/ and not inside it, because the benchmark stamps its recorded counter traffic with a hash
// of every file in csrc/; libksa.so keeps its own copies of fail, HIP_OK and DeviceGuard there.
//
// Everything here has internal linkage, and has to: the libraries are loaded into one process, and a symbol of default
// visibility (an inline thread-local above all) would be unified across them by the dynamic loader, so that one library's
// k??_last_error() returned another's message.  Each library that includes this file gets its own g_err.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <string>

namespace {

thread_local std::string g_err;

int fail(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return 1;
}

#define HIP_OK(call)                                                                      \
  do {                                                                                    \
    hipError_t _e = (call);                                                               \
    if (_e != hipSuccess) return fail("%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)

// Entry points run on their object's device and hand the caller's current device back on every exit path.
struct DeviceGuard {
  int prev = -1;
  DeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// outputs of a decimator by D for the next n samples of a stream that has taken `seen`: one per multiple of D it passes
long long stream_outputs(long long seen, long long n, long long D) { return ceil_div(seen + n, D) - ceil_div(seen, D); }

int check_taps(int T, const float* taps) {
  if (!taps) return fail("null taps pointer");
  for (int k = 0; k < T; ++k)
    if (!std::isfinite(taps[k])) return fail("tap %d is not finite", k);
  return 0;
}

// bytes of one I,Q pair in the sample formats every header numbers alike: complex64 0, uint8 1, int8 2, int16 3
int iq_sample_bytes(int fmt) { return fmt == 0 ? 8 : fmt == 3 ? 4 : 2; }

// the checks of k??_create that read alike in every library, with the one text each: the format first, the other two last
// before the first HIP call.  A library that calls the first two asserts that its header's K??_FMT_* are these numbers.
int check_iq_format(int fmt) { return fmt < 0 || fmt > 3 ? fail("unknown sample format %d", fmt) : 0; }

int check_u8_scaling(int fmt, float u8_offset, float u8_scale) {   // only the uint8 format reads the two
  if (fmt != 1) return 0;
  if (!std::isfinite(u8_scale) || u8_scale == 0.f) return fail("u8_scale %g must be finite and non-zero", (double)u8_scale);
  if (!std::isfinite(u8_offset)) return fail("u8_offset %g must be finite", (double)u8_offset);
  return 0;
}

int check_device(int device) { return device < 0 ? fail("device %d must be >= 0", device) : 0; }

int check_iq_aligned(const void* iq, int bytes) {
  if (reinterpret_cast<uintptr_t>(iq) % (unsigned)bytes) return fail("input pointer is not aligned to the %d bytes of a sample", bytes);
  return 0;
}

int cu_count(int device, int* cus) {
  if (hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || *cus < 1)
    return fail("hipDeviceGetAttribute(MultiprocessorCount) failed on device %d", device);
  return 0;
}

// k??_set_stream after its null check: work enqueued on the old stream is ordered before what follows on the new one
int hand_over_stream(int device, hipStream_t* stream, hipEvent_t* ev, void* hip_stream) {
  hipStream_t ns = reinterpret_cast<hipStream_t>(hip_stream);
  if (ns == *stream) return 0;
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(device));
  if (!*ev) HIP_OK(hipEventCreateWithFlags(ev, hipEventDisableTiming));
  HIP_OK(hipEventRecord(*ev, *stream));
  HIP_OK(hipStreamWaitEvent(ns, *ev, 0));
  *stream = ns;
  return 0;
}

// k??_synchronize after its null check
int synchronize_on(int device, hipStream_t stream) {
  DeviceGuard dev_guard;
  HIP_OK(hipSetDevice(device));
  HIP_OK(hipStreamSynchronize(stream));
  return 0;
}

// *buf holds at least `need` elements afterwards (*have counts them); a larger one replaces it once the stream's work on the
// old one is done.  The caller has set the device.
template <class T> int grow_device(T** buf, long long* have, long long need, hipStream_t stream) {
  if (*have >= need) return 0;
  HIP_OK(hipStreamSynchronize(stream));
  if (*buf) (void)hipFree(*buf);
  *buf = nullptr;
  *have = 0;
  HIP_OK(hipMalloc(reinterpret_cast<void**>(buf), (size_t)need * sizeof(T)));
  *have = need;
  return 0;
}

void free_device(std::initializer_list<void*> ptrs) {
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
}

}  // namespace
