/* libksa_ddc -- C ABI of the digital down-converter (zoom) front end on the MI355X (gfx950): a companion of libksa.
 *
 * A down-converter object shifts a frequency of interest to 0 Hz, low-pass filters and decimates by D: a time-domain
 * preprocessor whose output, a complex64 IQ block in device memory, is what ksa_frames_dev, ksa_curscan_dev and the scan entry
 * points of libksa already accept.  Analysing it with the same fft_size gives D times finer bins.  It shares no symbol, no
 * state and no header with libksa, libksa_density or libksa_mask.  The reference (hanishkvc/prgs-sdr-kspecanal) lists the stage
 * as a TODO and has no counterpart.
 *
 * Conventions are those of the other headers: plain C types only; 0 = success, non-zero = error with text in
 * kdc_last_error() (thread local).  "host" pointers are ordinary CPU memory, "dev" pointers are HIP device memory of the
 * object's device (or page-locked mapped host memory, e.g. from ksa_host_alloc).  One object = one GPU; no concurrent calls on
 * one object.  All device work is enqueued on the object's stream (kdc_set_stream); entry points that take or fill host memory
 * synchronise that stream before returning, the `_dev` ones do not synchronise.  Every entry point selects its object's device
 * for its own duration and hands the caller's current HIP device back on return.  The library reads no environment variable.
 * Argument checks come before any HIP call.  A hipStream_t travels as void*.
 *
 * Semantics (the contract of every layer):
 *
 * The object is created with:
 * - device.
 * - fmt: the sample format of the input, interleaved I,Q, little-endian.  The values and unpack rules are those of ksa.h:
 *     KDC_FMT_C64 = 0  float32 pairs, 8 bytes per sample, taken as they are
 *     KDC_FMT_U8  = 1  uint8 pairs, 2 bytes per sample, (b - u8_offset) * (1 / u8_scale); 1 / u8_scale is rounded to float32
 *                      once; ksa_config's defaults are 127.5 / 127.5
 *     KDC_FMT_S8  = 2  int8 pairs, 2 bytes per sample, b / 128
 *     KDC_FMT_S16 = 3  int16 pairs, 4 bytes per sample, b / 32768
 *   u8_offset and u8_scale are only read for KDC_FMT_U8.  An input pointer is aligned to its sample size (8, 2, 2, 4 bytes).
 * - decim D, 1 .. 1024.
 * - ntaps T, 1 .. 16384, and taps_host float32[T], the real FIR h.
 * - phase_inc: uint64, the mixer's step in turns per input sample, 2^64 = one turn.
 * - max_in: the largest number of input samples per call, 1 .. 2^28 - 1 (max_in * 8 < 2^31 as in ksa.h: offsets inside one
 *   call are 32-bit; the start of a block, b * block_stride, is formed in 64 bits).
 * Refused, with their own text and a null handle: D, T or max_in out of range, null taps, a non-finite tap, an unknown
 * format, a zero or non-finite u8_scale or a non-finite u8_offset (KDC_FMT_U8), a negative device.
 *
 * The object owns on the device an output buffer of max(ceil(max_in / D), max_in / T) + 1 complex64 values, which holds the
 * result of any permitted call (kdc_out_dev), the taps and T - 1 history samples.  The host object holds the rest of the stream
 * state: the uint64 phase accumulator and the int64 counts of samples in and out.
 *
 * Mixer.  v[n] = x[n] * w(phi_n), phi_(n+1) = phi_n + phase_inc in wrapping 64-bit integer arithmetic: exact for any stream
 * length, no float phase is ever accumulated.  w(phi) = (cos 2 pi phi, -sin 2 pi phi) in float32, so a signal at +f lands at
 * 0 Hz for phase_inc = round(f / fs * 2^64).  The angle is the top 32 bits of phi (2^-32 turn, truncated), split into the
 * nearest quarter turn and a remainder in [-1/8, 1/8) turn; the remainder is rounded to float32 (no coarser than 2^-27 turn).
 * Where the remainder is zero w is exactly (1,0), (0,-1), (-1,0), (0,1) and the product is a swap and a sign change:
 * phase_inc = 0 passes the samples through bit for bit.  Elsewhere sin and cos are polynomials on [-pi/4, pi/4] (about one ulp)
 * and v = (xr*wr - xi*wi, xr*wi + xi*wr), each with one fused multiply-add.  v[n] is a function of x[n] and phi_n alone.
 *
 * Stream form (kdc_process_dev, kdc_process): one continuous stream cut into calls.
 *   y[m] = sum_{k<T} h[k] * v[m*D - k],   v[n] = 0 for n < 0
 * Output m exists once input m*D has arrived: a call that brings the total from N0 to N1 samples yields
 * ceil(N1 / D) - ceil(N0 / D) outputs (kdc_out_count tells in advance); n_in = 0 is a successful no-op.  The outputs do not
 * depend on how the stream is cut into calls, bit for bit: real and imaginary parts are two float32 sums of fused
 * multiply-adds whose order is a function of k alone (of D and T through the kernel form, never of tile, call or grid).
 *
 * Block form (kdc_blocks_dev): nblocks independent captures, the engine's unit.  Block b starts at iq_dev + b * block_stride
 * samples (any stride >= 0, blocks may overlap), block_len >= T, nblocks * block_len <= max_in, the phase restarts at 0 in
 * every block and the stream state is neither read nor touched.
 *   out[b][m] = sum_{k<T} h[k] * v_b[m*D + (T-1) - k],   m < M = (block_len - T) / D + 1
 * Only outputs whose whole support lies inside the block are produced: no start-up transient, and
 * block_len = D * (full_size - 1) + T gives exactly full_size outputs.  Output b, m goes to out_dev[b * out_stride + m]
 * (out_stride >= M); out_dev = NULL writes the object's own buffer at out_stride = M.
 *
 * There are no float atomics, and no result depends on the grid.
 *
 * Refused per call, each with its own text and leaving the object as it was: a null object or input pointer (with n > 0), a
 * misaligned input pointer, a negative count, more than max_in samples, block_len < T, a negative stride, out_stride < M, an
 * output capacity too small for the call's outputs.
 */
#ifndef KSA_DDC_H
#define KSA_DDC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KDC_ABI_VERSION 1 /* A binding takes the number from kdc_abi_version() of the library it loaded. */
#define KDC_FMT_C64 0
#define KDC_FMT_U8 1
#define KDC_FMT_S8 2
#define KDC_FMT_S16 3
#define KDC_MAX_DECIM 1024
#define KDC_MAX_TAPS 16384
#define KDC_MAX_IN 268435455 /* 2^28 - 1 */
/* kernel forms reported by kdc_kernel_info */
#define KDC_FORM_TILE 0   /* one output per thread and register block, the tile's span in LDS, D phases side by side */
#define KDC_FORM_REDUCE 1 /* long dot products spread over the workgroup's lanes, the span walked in chunks */

typedef struct kdc_ddc kdc_ddc;

int kdc_abi_version(void);
const char* kdc_last_error(void);

/* A down-converter on `device` with zero history, phase 0 and zero counts, its stream the NULL stream.  *out is NULL when
 * refused. */
int kdc_create(int32_t device, int32_t fmt, float u8_offset, float u8_scale, int32_t decim, int32_t ntaps,
               const float* taps_host, uint64_t phase_inc, int64_t max_in, kdc_ddc** out);
void kdc_destroy(kdc_ddc* h);

/* Same ordering rule as ksm_set_stream: work already enqueued on the old stream is ordered in front of work on the new one
 * (an event is recorded on the OLD stream, so a stream handed in here must stay alive until the next kdc_set_stream /
 * kdc_destroy of this object). */
int kdc_set_stream(kdc_ddc* h, void* hip_stream);
int kdc_synchronize(kdc_ddc* h);

/* The number of outputs the next stream call of n_in samples yields: ceil((N0 + n_in) / D) - ceil(N0 / D). */
int kdc_out_count(kdc_ddc* h, int64_t n_in, int64_t* n_out);
/* The next n_in samples of the stream from device memory.  The outputs go to out_dev[0 .. *n_out) (complex64,
 * out_capacity values), or with out_dev = NULL to the object's own buffer (out_capacity is ignored).  n_out may be NULL.
 * Asynchronous. */
int kdc_process_dev(kdc_ddc* h, const void* iq_dev, int64_t n_in, void* out_dev, int64_t out_capacity, int64_t* n_out);
/* The same from host memory into host memory (out_host complex64[out_capacity]); staged through library-owned device memory;
 * synchronises. */
int kdc_process(kdc_ddc* h, const void* iq_host, int64_t n_in, void* out_host, int64_t out_capacity, int64_t* n_out);
/* The block form.  block_stride and block_len in samples, out_stride in complex64 values.  Asynchronous. */
int kdc_blocks_dev(kdc_ddc* h, const void* iq_dev, int64_t block_stride, int64_t nblocks, int64_t block_len, void* out_dev,
                   int64_t out_stride);

/* A new phase_inc from the next input sample on; the phase stays continuous. */
int kdc_set_tuning(kdc_ddc* h, uint64_t phase_inc);
/* Replace the T taps (the same checks as kdc_create); outputs already enqueued use the old taps, the history is kept.
 * Synchronises. */
int kdc_set_taps(kdc_ddc* h, const float* taps_host);
/* History, counts and phase to zero.  Asynchronous. */
int kdc_reset(kdc_ddc* h);
/* Samples in, samples out and the phase of the next input sample; any out pointer may be NULL.  No device work. */
int kdc_state(kdc_ddc* h, int64_t* samples_in, int64_t* samples_out, uint64_t* phase);
/* The object's output buffer (complex64[*capacity]), valid until kdc_destroy: zero-copy for torch.  capacity may be NULL. */
int kdc_out_dev(kdc_ddc* h, void** out_dev, int64_t* capacity);

/* The filter kernel of the last launch (before any: of this object's D and T, with a grid that fills the device): threads
 * per workgroup, LDS bytes per workgroup (static and dynamic), VGPRs, workgroups, outputs per workgroup, and form =
 * KDC_FORM_TILE or KDC_FORM_REDUCE.  The form and the outputs per workgroup depend on D and T alone.  Any out pointer may be
 * NULL. */
int kdc_kernel_info(kdc_ddc* h, int32_t* threads, int32_t* lds_bytes, int32_t* vgprs, int32_t* grid, int32_t* tile_out,
                    int32_t* form);

#ifdef __cplusplus
}
#endif

#endif
