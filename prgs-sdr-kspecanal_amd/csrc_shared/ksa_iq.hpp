// How interleaved I,Q of the four sample formats becomes float2 on the device, for the companion kernels that read raw samples
// (csrc_ddc/, csrc_chan/).  Every arithmetic step is spelled with an explicit rounding intrinsic, so that a history kernel and
// a loader give the same bits for the same sample.  A is the kernel's argument struct; only its u8_offset and u8_inv_scale
// are read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ksa {
namespace iq {

constexpr int FMT_C64 = 0, FMT_U8 = 1, FMT_S8 = 2, FMT_S16 = 3;

template <int FMT> struct Fmt { static constexpr int BYTES = FMT == FMT_C64 ? 8 : FMT == FMT_S16 ? 4 : 2; static constexpr int PER_VEC = 16 / BYTES; };

template <class A> __device__ __forceinline__ float2 unpack_u8(unsigned h, const A& a) {
  return make_float2(__fmul_rn(__fsub_rn((float)(h & 0xffu), a.u8_offset), a.u8_inv_scale),
                     __fmul_rn(__fsub_rn((float)((h >> 8) & 0xffu), a.u8_offset), a.u8_inv_scale));
}
__device__ __forceinline__ float2 unpack_s8(unsigned h) {
  return make_float2(__fmul_rn((float)(int)(signed char)(h & 0xffu), 0.0078125f),
                     __fmul_rn((float)(int)(signed char)((h >> 8) & 0xffu), 0.0078125f));
}
__device__ __forceinline__ float2 unpack_s16(unsigned w) {
  return make_float2(__fmul_rn((float)(int)(short)(w & 0xffffu), 0.000030517578125f),
                     __fmul_rn((float)(int)(short)(w >> 16), 0.000030517578125f));
}

// sample e of the 16 bytes w
template <int FMT, class A> __device__ __forceinline__ float2 sample_of(const uint4& w, int e, const A& a) {
  const unsigned d[4] = {w.x, w.y, w.z, w.w};
  if (FMT == FMT_C64) return make_float2(__uint_as_float(d[2 * e]), __uint_as_float(d[2 * e + 1]));
  if (FMT == FMT_S16) return unpack_s16(d[e]);
  const unsigned h = (d[e >> 1] >> (16 * (e & 1))) & 0xffffu;
  return FMT == FMT_U8 ? unpack_u8(h, a) : unpack_s8(h);
}

// raw sample r of the block at base
template <int FMT, class A> __device__ __forceinline__ float2 sample_at(const char* base, int r, const A& a) {
  if (FMT == FMT_C64) {
    const uint2 w = *reinterpret_cast<const uint2*>(base + (size_t)r * 8);
    return make_float2(__uint_as_float(w.x), __uint_as_float(w.y));
  }
  if (FMT == FMT_S16) return unpack_s16(*reinterpret_cast<const unsigned*>(base + (size_t)r * 4));
  const unsigned h = *reinterpret_cast<const unsigned short*>(base + (size_t)r * 2);
  return FMT == FMT_U8 ? unpack_u8(h, a) : unpack_s8(h);
}

}  // namespace iq
}  // namespace ksa
