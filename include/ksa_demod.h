/* libksa_demod -- C ABI of the AM / FM / PM demodulator behind the zoom on the MI355X (gfx950): a companion of libksa.
 *
 * A demodulator object turns a complex64 IQ block in device memory -- what kdc_out_dev of libksa_ddc holds after the zoom, or
 * a raw complex64 capture -- into a real signal versus time: amplitude (AM), frequency (FM) or phase (PM) per sample, low-pass
 * filtered by a real FIR and decimated by D, as float32 or as int16 PCM.  It shares no symbol, no state and no header with
 * libksa, libksa_density, libksa_mask, libksa_ddc or libksa_detect.  The reference (hanishkvc/prgs-sdr-kspecanal) has no
 * counterpart.
 *
 * Conventions are those of the other headers: plain C types only; 0 = success, non-zero = error with text in
 * kdm_last_error() (thread local).  "host" pointers are ordinary CPU memory, "dev" pointers are HIP device memory of the
 * object's device (or page-locked mapped host memory).  One object = one GPU; no concurrent calls on one object.  All device
 * work is enqueued on the object's stream (kdm_set_stream); entry points that take or fill host memory synchronise that stream
 * before returning, the `_dev` ones do not synchronise.  Every entry point selects its object's device for its own duration
 * and hands the caller's current HIP device back on return.  The library reads no environment variable.  Argument checks come
 * before any HIP call.  A hipStream_t travels as void*.
 *
 * Semantics (the contract of every layer):
 *
 * The object is created with:
 * - device.
 * - mode: KDM_MODE_AM = 0, KDM_MODE_FM = 1, KDM_MODE_PM = 2.
 * - decim D, 1 .. 256.
 * - ntaps T, 1 .. 4096, and taps_host float32[T], the real FIR h.
 * - out_fmt: KDM_OUT_F32 = 0 (float32 outputs) or KDM_OUT_S16 = 1 (int16 PCM); pcm_scale is only read for KDM_OUT_S16.
 * - max_in: the largest number of input samples per call, 1 .. 2^28 - 1 (offsets inside one call are 32-bit; the start of a
 *   block, b * block_stride, is formed in 64 bits).
 * The input is always complex64, interleaved float32 I,Q, and an input pointer is aligned to 8 bytes.
 * Refused, with their own text and a null handle: an unknown mode or output format, D, T or max_in out of range, null taps, a
 * non-finite tap, a pcm_scale that is not finite and > 0 (KDM_OUT_S16), a negative device.
 *
 * The object owns on the device an output buffer of max(ceil(max_in / D), max_in / T) + 1 values, which holds the result of
 * any permitted call (kdm_out_dev, kdm_read_out), the taps, T - 1 already demodulated history samples and the last raw sample
 * of the stream.  The host object holds the rest of the stream state: the int64 counts of samples in and out.
 *
 * Detector.  d[n], float32, is a function of x[n] and x[n-1] alone:
 *   AM  d = sqrtf(fmaf(re, re, im * im)): the product and the square root correctly rounded
 *   PM  d = turns(re, im) of x[n]
 *   FM  p = x[n] * conj(x[n-1]): pr = fmaf(xr, yr, xi * yi), pi = fmaf(xi, yr, -(xr * yi)), each inner product rounded once,
 *       d = turns(pr, pi); x[-1] = 0 at the start of a stream, after kdm_reset and at the start of every block
 * turns(re, im) is atan2f(im, re) times float32(1 / 2 pi), in [-0.5, 0.5], and exact on the axes, where zero means either
 * sign of zero: both zero -> 0; im == 0 and re > 0 -> 0; im == 0 and re < 0 -> +0.5; re == 0 and im > 0 -> +0.25; re == 0 and
 * im < 0 -> -0.25.  So FM gives the frequency in cycles per input sample and PM the phase in cycles.  The same sample gives
 * the same bits on every path of the library.  Non-finite input gives unspecified values and traps nowhere.
 *
 * Stream form (kdm_process_dev, kdm_process): one continuous stream cut into calls.
 *   y[m] = sum_{k<T} h[k] * d[m*D - k],   d[n] = 0 for n < 0
 * Output m exists once input m*D has arrived: a call that brings the total from N0 to N1 samples yields
 * ceil(N1 / D) - ceil(N0 / D) outputs (kdm_out_count tells in advance); n_in = 0 is a successful no-op.  The outputs do not
 * depend on how the stream is cut into calls, bit for bit: every output is one float32 chain of fused multiply-adds whose
 * order is a function of k alone (never of tile, call or grid).
 *
 * Block form (kdm_blocks_dev): nblocks independent captures, the engine's unit.  Block b starts at iq_dev + b * block_stride
 * samples (any stride >= 0, blocks may overlap); the stream state is neither read nor touched.  lead = 1 for FM (the first
 * sample of a block has no predecessor), else 0; block_len >= T + lead, nblocks * block_len <= max_in.
 *   out[b][m] = sum_{k<T} h[k] * d_b[lead + m*D + (T-1) - k],   m < M = (block_len - lead - T) / D + 1
 * Only outputs whose whole support lies inside the block are produced: no start-up transient.  Output b, m goes to
 * out_dev[b * out_stride + m] (out_stride >= M, in values); out_dev = NULL writes the object's own buffer at out_stride = M.
 *
 * Output.  KDM_OUT_F32 stores y.  KDM_OUT_S16 stores (int16) min(max(rintf(y * pcm_scale), -32768), 32767); NaN becomes 0.
 *
 * There are no float atomics, and no result depends on the grid.
 *
 * Refused per call, each with its own text and leaving the object as it was: a null object or input pointer (with n > 0), a
 * misaligned input pointer, a negative count, more than max_in samples, block_len < T + lead, a negative stride,
 * out_stride < M, an output capacity too small for the call's outputs.  A failure of the HIP runtime inside a call is another
 * matter: if a stream call's second launch (the history) fails after its first (the filter), outputs may have been written
 * while history and counts have not moved; the object then refuses further stream calls, with its own text, until kdm_reset.
 * The block form has one launch and no such state.
 */
#ifndef KSA_DEMOD_H
#define KSA_DEMOD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KDM_ABI_VERSION 1 /* A binding takes the number from kdm_abi_version() of the library it loaded. */
#define KDM_MODE_AM 0
#define KDM_MODE_FM 1
#define KDM_MODE_PM 2
#define KDM_OUT_F32 0
#define KDM_OUT_S16 1
#define KDM_MAX_DECIM 256
#define KDM_MAX_TAPS 4096
#define KDM_MAX_IN 268435455 /* 2^28 - 1 */

typedef struct kdm_demod kdm_demod;

int kdm_abi_version(void);
const char* kdm_last_error(void);

/* A demodulator on `device` with zero history, a zero last sample and zero counts, its stream the NULL stream.  *out is NULL
 * when refused. */
int kdm_create(int32_t device, int32_t mode, int32_t decim, int32_t ntaps, const float* taps_host, int32_t out_fmt,
               float pcm_scale, int64_t max_in, kdm_demod** out);
void kdm_destroy(kdm_demod* h);

/* Work already enqueued on the old stream is ordered in front of work on the new one (an event is recorded on the OLD stream,
 * so a stream handed in here must stay alive until the next kdm_set_stream / kdm_destroy of this object). */
int kdm_set_stream(kdm_demod* h, void* hip_stream);
int kdm_synchronize(kdm_demod* h);

/* The number of outputs the next stream call of n_in samples yields: ceil((N0 + n_in) / D) - ceil(N0 / D). */
int kdm_out_count(kdm_demod* h, int64_t n_in, int64_t* n_out);
/* The next n_in samples of the stream from device memory.  The outputs go to out_dev[0 .. *n_out) (float32 or int16,
 * out_capacity values), or with out_dev = NULL to the object's own buffer (out_capacity is ignored).  n_out may be NULL.
 * Asynchronous. */
int kdm_process_dev(kdm_demod* h, const void* iq_dev, int64_t n_in, void* out_dev, int64_t out_capacity, int64_t* n_out);
/* The same from host memory into host memory (out_host float32 or int16 [out_capacity]); staged through library-owned device
 * memory; synchronises. */
int kdm_process(kdm_demod* h, const void* iq_host, int64_t n_in, void* out_host, int64_t out_capacity, int64_t* n_out);
/* The block form.  block_stride and block_len in samples, out_stride in output values.  Asynchronous. */
int kdm_blocks_dev(kdm_demod* h, const void* iq_dev, int64_t block_stride, int64_t nblocks, int64_t block_len, void* out_dev,
                   int64_t out_stride);

/* Replace the T taps (the same checks as kdm_create); outputs already enqueued use the old taps, the history is kept.
 * Synchronises. */
int kdm_set_taps(kdm_demod* h, const float* taps_host);
/* History, last sample and counts to zero.  Asynchronous. */
int kdm_reset(kdm_demod* h);
/* Samples in and samples out of the stream; any out pointer may be NULL.  No device work. */
int kdm_state(kdm_demod* h, int64_t* samples_in, int64_t* samples_out);
/* The object's output buffer (float32 or int16 [*capacity]), valid until kdm_destroy: zero-copy for torch.  capacity may be
 * NULL. */
int kdm_out_dev(kdm_demod* h, void** out_dev, int64_t* capacity);
/* Values [first, first + count) of the object's output buffer to out_host (float32 or int16 [count]); synchronises. */
int kdm_read_out(kdm_demod* h, void* out_host, int64_t first, int64_t count);

/* The filter kernel of the last launch (before any: of this object's D and T, with a grid that fills the device): threads
 * per workgroup, LDS bytes per workgroup (static and dynamic), VGPRs, workgroups and outputs per workgroup.  The outputs per
 * workgroup depend on D and T alone.  Any out pointer may be NULL. */
int kdm_kernel_info(kdm_demod* h, int32_t* threads, int32_t* lds_bytes, int32_t* vgprs, int32_t* grid, int32_t* tile_out);

#ifdef __cplusplus
}
#endif

#endif
