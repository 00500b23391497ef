// Polyphase filter bank front end (KSA_CUMU_PFB): the time-domain fold in front of the transform.
//   y[f][n] = sum over k < P, in the order k = 0, 1, ..., of x[f*frame_stride + starts[k] + n] * taps[k*N + n]
// written as complex64 [frames][N] into engine scratch; the engine's spectrum kernels then transform y with one window at
// start 0 and an all-ones tap table (ksa_api.hip: run_spectrum).  Two kernels, one arithmetic: every output point starts from
// acc = 0 and takes acc = fmaf(x_k, taps_k, acc) per component in tap order, on samples converted exactly as their format is
// defined (pfb_sample), so the two agree bit for bit.
//   pfb_fold_kernel<FMT>      any starts, any stride, any P: P loads per output point.
//   pfb_ring_kernel<FMT, P>   frame_stride == N, starts[k] == k*N and pfb_ring_pays(FMT, P) (the critically sampled PFB): frame f is the segments
//                             f .. f+P-1 of one sample stream, so consecutive frames share P-1 of them.  A thread keeps its
//                             columns' P taps and the last P segments in registers and walks PFB_SLICE_FRAMES frames: one new
//                             load per output point, P-1 warm-up loads per slice.  The frame loop is unrolled by P, which makes
//                             every ring index a compile-time constant (no scratch).
// A thread owns PFB_COLS adjacent columns: one 16-byte store per frame, one 16 / 8 / 4-byte load per segment.
//
// Integrating polyphase spectrometer (KSA_CUMU_PFB_PSD): a block holds K sub-frames that advance by N samples,
//   y[b*K + j][n] = sum over k < P of x[b*frame_stride + j*N + starts[k] + n] * taps[k*N + n]            j = 0 .. K-1
// written as complex64 [blocks*K][N]; the transform stage then runs its PSD instantiations over every block as ONE frame of K
// rectangular windows at hop N.  The same arithmetic in two block-aware kernels:
//   pfbpsd_fold_kernel<FMT>      any starts, any stride, any P.
//   pfbpsd_ring_kernel<FMT, P>   starts[k] == k*N and pfbpsd_ring_pays(FMT, P) (P = 4, 8, 16): the sliding happens INSIDE a block, whatever
//                                frame_stride is; a thread walks one slice of at most PFB_SLICE_FRAMES sub-frames of one block.
#pragma once
#include <hip/hip_runtime.h>

#include "ksa_kernels.hpp"

namespace ksa {

constexpr int PFB_SLICE_FRAMES = 32;   // frames one ring-kernel thread walks (warm-up cost (P-1)/32 loads per output point)
constexpr int PFB_COLS = 2;            // adjacent columns per thread: 2 x float2 = one 16-byte store
constexpr int PFB_THREADS = 256;

// Where the ring kernel ships: where it measured faster than the generic kernel at stride N (profiles/pfb_sweep.txt).  It
// saves (P - 1) re-reads of a sample per output point and pays with P - 1 warm-up loads per slice and fewer, longer threads:
// from 12 saved bytes up it won (complex64 P >= 4, 2-byte samples P >= 8); below, the generic kernel's re-reads hit in cache.
// Only these (format, P) pairs are instantiated.
__host__ __device__ constexpr bool pfb_ring_pays(int fmt, int taps) {
  return (taps == 4 || taps == 8 || taps == 16) && (taps - 1) * fmt_bytes(fmt) >= 12;
}

struct PfbParams {
  const void* iq;           // samples of format FMT; frame f starts at sample f*frame_stride
  long long frame_stride;   // samples
  int nframes;
  int n;                    // fft_size (a multiple of 4)
  int ntaps;                // P
  const int* starts;        // [P] segment starts inside a frame (generic kernel)
  const float* taps;        // [P][N]
  float u8_offset, u8_inv_scale;
  float2* y;                // [nframes][N]
};

typedef float pfb_f4 __attribute__((ext_vector_type(4)));

// PFB_COLS adjacent samples starting at sample index s, converted as the format defines:
// s8 b/128, s16 b/32768, u8 (b - offset) * (1/scale), complex64 as is.  Returned as {re0, im0, re1, im1}.
template <int FMT>
__device__ __forceinline__ pfb_f4 pfb_sample(const PfbParams& a, long long s) {
  pfb_f4 v;
  if constexpr (FMT == FMT_C64) {
    // (a sample stream is 8-byte aligned only: two 8-byte loads, which the compiler may merge where it can prove more)
    const float2* p = static_cast<const float2*>(a.iq) + s;
    const float2 lo = p[0], hi = p[1];
    v = pfb_f4{lo.x, lo.y, hi.x, hi.y};
  } else if constexpr (FMT == FMT_S16) {
    const unsigned* p = static_cast<const unsigned*>(a.iq) + s;
    const float2 lo = unpack_signed<FMT_S16>(p[0]), hi = unpack_signed<FMT_S16>(p[1]);
    v = pfb_f4{lo.x, lo.y, hi.x, hi.y} * fmt_fixed_scale(FMT_S16);
  } else if constexpr (FMT == FMT_S8) {
    const unsigned short* p = static_cast<const unsigned short*>(a.iq) + s;
    const float2 lo = unpack_signed<FMT_S8>(p[0]), hi = unpack_signed<FMT_S8>(p[1]);
    v = pfb_f4{lo.x, lo.y, hi.x, hi.y} * fmt_fixed_scale(FMT_S8);
  } else {
    const unsigned short* p = static_cast<const unsigned short*>(a.iq) + s;
    const unsigned b0 = p[0], b1 = p[1];
    v = pfb_f4{(float)(b0 & 0xff), (float)(b0 >> 8), (float)(b1 & 0xff), (float)(b1 >> 8)};
    v = (v - a.u8_offset) * a.u8_inv_scale;
  }
  return v;
}

// acc += x * w per component, w = the taps of the two columns
__device__ __forceinline__ pfb_f4 pfb_mac(pfb_f4 acc, pfb_f4 x, float2 w) {
  acc.x = fmaf(x.x, w.x, acc.x);
  acc.y = fmaf(x.y, w.x, acc.y);
  acc.z = fmaf(x.z, w.y, acc.z);
  acc.w = fmaf(x.w, w.y, acc.w);
  return acc;
}

// One work item = PFB_COLS adjacent columns of one frame; items are numbered frame-major and walked in grid strides, so that
// a wave reads adjacent columns (and, where N is small, adjacent frames).
template <int FMT>
__global__ __launch_bounds__(PFB_THREADS) void pfb_fold_kernel(const PfbParams a) {
  const int per = a.n / PFB_COLS;
  const long long items = (long long)a.nframes * per;
  for (long long i = (long long)blockIdx.x * PFB_THREADS + threadIdx.x; i < items; i += (long long)gridDim.x * PFB_THREADS) {
    const int f = (int)(i / per), col = (int)(i - (long long)f * per) * PFB_COLS;
    const long long base = (long long)f * a.frame_stride + col;
    pfb_f4 acc = pfb_f4{0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < a.ntaps; ++k) {
      const float2 w = *reinterpret_cast<const float2*>(a.taps + (size_t)k * a.n + col);
      acc = pfb_mac(acc, pfb_sample<FMT>(a, base + a.starts[k]), w);
    }
    *reinterpret_cast<pfb_f4*>(a.y + (size_t)f * a.n + col) = acc;
  }
}

// One work item = PFB_COLS adjacent columns of one slice of PFB_SLICE_FRAMES frames, numbered slice-major; one item per thread
// (grid = ceil(items / PFB_THREADS)).  Segment s of the stream = samples [s*N, (s+1)*N); frame f folds segments f .. f+P-1.
template <int FMT, int P>
__global__ __launch_bounds__(PFB_THREADS) void pfb_ring_kernel(const PfbParams a) {
  const int per = a.n / PFB_COLS;
  const long long i = (long long)blockIdx.x * PFB_THREADS + threadIdx.x;
  const int slice = (int)(i / per), col = (int)(i - (long long)slice * per) * PFB_COLS;
  const int f0 = slice * PFB_SLICE_FRAMES, f1 = min(f0 + PFB_SLICE_FRAMES, a.nframes);
  if (f0 >= a.nframes) return;
  float2 w[P];
#pragma unroll
  for (int k = 0; k < P; ++k) w[k] = *reinterpret_cast<const float2*>(a.taps + (size_t)k * a.n + col);
  pfb_f4 ring[P];     // segment f0 + j lives in ring[j % P]
#pragma unroll
  for (int j = 0; j < P - 1; ++j) ring[j] = pfb_sample<FMT>(a, (long long)(f0 + j) * a.n + col);
  for (int f = f0; f < f1; f += P) {
#pragma unroll
    for (int u = 0; u < P; ++u) {
      if (f + u < f1) {
        ring[(u + P - 1) % P] = pfb_sample<FMT>(a, (long long)(f + u + P - 1) * a.n + col);
        pfb_f4 acc = pfb_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < P; ++k) acc = pfb_mac(acc, ring[(u + k) % P], w[k]);
        *reinterpret_cast<pfb_f4*>(a.y + (size_t)(f + u) * a.n + col) = acc;
      }
    }
  }
}

// ---- KSA_CUMU_PFB_PSD: K sub-frames per block -------------------------------------------------------------------------------
// Where the block ring kernel ships: where it measured faster than the block generic kernel (profiles/pfbpsd_sweep.txt) -- every
// sample format at P = 4, 8, 16, the 2-byte formats at P = 4 included (1.70 x there, where pfb_ring_pays keeps the frame-wise
// ring kernel out: inside a block the ring form also spares the generic form's per-item index arithmetic, and it won down to
// K = 1, where both load the same samples).  Only these pairs are instantiated.
__host__ __device__ constexpr bool pfbpsd_ring_pays(int fmt, int taps) {
  return fmt >= FMT_C64 && fmt <= FMT_S16 && (taps == 4 || taps == 8 || taps == 16);
}

struct PfbPsdParams {
  PfbParams f;   // iq, frame_stride (between BLOCKS), nframes = blocks, n, ntaps, starts, taps, u8_*, y = [blocks*nsub][N]
  int nsub;      // K: sub-frames per block
};

// One work item = PFB_COLS adjacent columns of one (block, sub-frame), numbered row-major over [blocks*K][N / PFB_COLS] and
// walked in grid strides: a wave reads adjacent columns.
template <int FMT>
__global__ __launch_bounds__(PFB_THREADS) void pfbpsd_fold_kernel(const PfbPsdParams a) {
  const int per = a.f.n / PFB_COLS;
  const long long items = (long long)a.f.nframes * a.nsub * per;
  for (long long i = (long long)blockIdx.x * PFB_THREADS + threadIdx.x; i < items; i += (long long)gridDim.x * PFB_THREADS) {
    const int row = (int)(i / per), col = (int)(i - (long long)row * per) * PFB_COLS;
    const int b = row / a.nsub, j = row - b * a.nsub;
    const long long base = (long long)b * a.f.frame_stride + (long long)j * a.f.n + col;
    pfb_f4 acc = pfb_f4{0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < a.f.ntaps; ++k) {
      const float2 w = *reinterpret_cast<const float2*>(a.f.taps + (size_t)k * a.f.n + col);
      acc = pfb_mac(acc, pfb_sample<FMT>(a.f, base + a.f.starts[k]), w);
    }
    *reinterpret_cast<pfb_f4*>(a.f.y + (size_t)row * a.f.n + col) = acc;
  }
}

// One work item = PFB_COLS adjacent columns of one slice of at most PFB_SLICE_FRAMES sub-frames of one block, numbered
// (block, slice)-major; one item per thread.  Segment s of block b = samples [b*frame_stride + s*N, ... + N); sub-frame j folds
// segments j .. j+P-1.  K need be no multiple of P or of the slice: the unrolled trip is guarded per sub-frame.
template <int FMT, int P>
__global__ __launch_bounds__(PFB_THREADS) void pfbpsd_ring_kernel(const PfbPsdParams a) {
  const int per = a.f.n / PFB_COLS;
  const int slices = (a.nsub + PFB_SLICE_FRAMES - 1) / PFB_SLICE_FRAMES;
  const long long i = (long long)blockIdx.x * PFB_THREADS + threadIdx.x;
  const int bs = (int)(i / per), col = (int)(i - (long long)bs * per) * PFB_COLS;
  const int b = bs / slices, slice = bs - b * slices;
  if (b >= a.f.nframes) return;
  const int f0 = slice * PFB_SLICE_FRAMES, f1 = min(f0 + PFB_SLICE_FRAMES, a.nsub);
  const long long x0 = (long long)b * a.f.frame_stride + col;     // the block's segment 0, this thread's columns
  float2* const y = a.f.y + ((size_t)b * a.nsub) * a.f.n + col;
  float2 w[P];
#pragma unroll
  for (int k = 0; k < P; ++k) w[k] = *reinterpret_cast<const float2*>(a.f.taps + (size_t)k * a.f.n + col);
  pfb_f4 ring[P];     // segment f0 + j lives in ring[j % P]
#pragma unroll
  for (int j = 0; j < P - 1; ++j) ring[j] = pfb_sample<FMT>(a.f, x0 + (long long)(f0 + j) * a.f.n);
  for (int f = f0; f < f1; f += P) {
#pragma unroll
    for (int u = 0; u < P; ++u) {
      if (f + u < f1) {
        ring[(u + P - 1) % P] = pfb_sample<FMT>(a.f, x0 + (long long)(f + u + P - 1) * a.f.n);
        pfb_f4 acc = pfb_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < P; ++k) acc = pfb_mac(acc, ring[(u + k) % P], w[k]);
        *reinterpret_cast<pfb_f4*>(y + (size_t)(f + u) * a.f.n) = acc;
      }
    }
  }
}

}  // namespace ksa
