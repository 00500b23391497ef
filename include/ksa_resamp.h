/* libksa_resamp -- C ABI of the rational (polyphase L / M) resampler on the MI355X (gfx950): a companion of libksa.
 *
 * A resampler object turns a stream or a set of blocks in device memory -- real float32, what kdm_ of libksa_demod leaves with
 * KDM_OUT_F32, or interleaved complex64, what kdc_out_dev of libksa_ddc and kch_out_dev of libksa_chan hold -- into the same
 * signal at L / M times the rate: zero-stuff by L, filter by the FIR h, keep every M-th.  It is the stage that decouples the
 * output rate from the capture rate; the integer stages in front do the heavy decimation, this one the last ratio.  It shares
 * no symbol, no state and no header with libksa or the other companions.  The reference (hanishkvc/prgs-sdr-kspecanal) has no
 * counterpart.
 *
 * Conventions are those of the other headers: plain C types only; 0 = success, non-zero = error with text in
 * krs_last_error() (thread local).  "host" pointers are ordinary CPU memory, "dev" pointers are HIP device memory of the
 * object's device (or page-locked mapped host memory).  One object = one GPU; no concurrent calls on one object.  All device
 * work is enqueued on the object's stream (krs_set_stream); entry points that take or fill host memory synchronise that stream
 * before returning, the `_dev` ones do not synchronise.  Every entry point selects its object's device for its own duration
 * and hands the caller's current HIP device back on return.  The library reads no environment variable.  Argument checks come
 * before any HIP call.  A hipStream_t travels as void*.
 *
 * Semantics (the contract of every layer):
 *
 * The object is created with:
 * - device.
 * - type: KRS_TYPE_F32 = 0 (real float32 samples, input pointers aligned to 4 bytes) or KRS_TYPE_C64 = 1 (interleaved complex64
 *   samples, input pointers aligned to 8 bytes).
 * - L, 1 .. 1024, and M, 1 .. 16384, with M <= 16 L and gcd(L, M) = 1: a pair that is not reduced is refused with a text that
 *   names the reduced pair.
 * - taps_per_phase P, 1 .. 256, with T = L P <= 16384, and taps_host float32[T], the real FIR h at the zero-stuffed rate.
 * - out_fmt: KRS_OUT_SAME = 0 (float32 or complex64, as the input) or KRS_OUT_S16 = 1 (int16 PCM, real input only); pcm_scale
 *   is only read for KRS_OUT_S16.
 * - max_in: the largest number of input samples per call, 1 .. 2^28 - 1 (sample offsets inside one call are 32-bit; the start
 *   of a block, b * block_stride, the position t = m M and every output count are formed in 64 bits).
 * Refused, with their own text and a null handle: an unknown type or output format, L, M, P, T or max_in out of range,
 * M > 16 L, a pair that is not reduced, KRS_OUT_S16 with complex input, null taps, a non-finite tap, a pcm_scale that is not
 * finite and > 0 (KRS_OUT_S16), a negative device.
 *
 * The object owns on the device an output buffer of ceil(max_in L / M) + 1 values (krs_out_dev, krs_read_out), the taps and
 * P - 1 raw history samples.  The host object holds the rest of the stream state: the int64 counts of samples in and out.
 *
 * Definition.  The stream's input is x[n], with x[n] = 0 for n < 0.  For output m >= 0:
 *   t = m M,  n = t div L,  p = t mod L
 *   y[m] = sum_{q<P} h[p + q L] * x[n - q]
 * Every output is one float32 chain of fused multiply-adds that starts at zero, q ascending; each part of a complex sample has
 * its own chain.  The order is a function of q alone, never of tile, call or grid.  This is zero-stuffing by L, filtering by h
 * and keeping every M-th value; in float64 it is np.convolve on the zero-stuffed input.
 *
 * Stream form (krs_process_dev, krs_process, krs_out_count): one continuous stream cut into calls.  Output m exists once input
 * n(m) has arrived: a call that brings the total from N0 to N1 samples yields ceil(N1 L / M) - ceil(N0 L / M) outputs
 * (krs_out_count tells in advance); n_in = 0 is a successful no-op.  The outputs do not depend on how the stream is cut into
 * calls, bit for bit.  The counts are int64 and the products with L and M cannot overflow, because a call that would take
 * samples_in past 2^52 is refused.  krs_reset_at(h, samples_in) zeroes the history and sets the counts as if that many zero
 * samples had been fed (samples_out = ceil(samples_in L / M)); krs_reset is krs_reset_at(h, 0).
 *
 * Block form (krs_blocks_dev): nblocks independent blocks.  Block b starts at in_dev + b * block_stride samples (any
 * stride >= 0, blocks may overlap); the phase restarts in every block, the stream state is neither read nor touched, and the
 * start-up transient is dropped: with first = ceil((P - 1) L / M),
 *   out[b][j] = y_b[first + j],   j < J = ceil(block_len L / M) - first
 * where y_b is the definition above on block b alone, so that every output's whole support lies inside the block.  A call
 * needs J >= 1 and nblocks * block_len <= max_in.  Output b, j goes to out_dev[b * out_stride + j] (out_stride >= J, in
 * values); out_dev = NULL writes the object's own buffer at out_stride = J.  A block that starts s samples into a stream
 * equals that stream's outputs bit for bit when s is a multiple of M: out[j] is then the stream's y[s L / M + first + j].
 *
 * Output.  KRS_OUT_SAME stores y.  KRS_OUT_S16 stores (int16) min(max(rintf(y * pcm_scale), -32768), 32767); NaN becomes 0.
 *
 * There are no float atomics, and no result depends on the grid or on the tile.
 *
 * Refused per call, each with its own text and leaving the object as it was: a null object or input pointer (with n > 0), a
 * misaligned input pointer, a negative count, more than max_in samples, J < 1, a negative stride, out_stride < J, an output
 * capacity too small for the call's outputs, a stream position past 2^52.  A failure of the HIP runtime inside a call is
 * another matter: if a stream call's second launch (the history) fails after its first (the filter), outputs may have been
 * written while history and counts have not moved; the object then refuses further stream calls, with its own text, until
 * krs_reset / krs_reset_at.  The block form has one launch and no such state.
 */
#ifndef KSA_RESAMP_H
#define KSA_RESAMP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KRS_ABI_VERSION 1 /* A binding takes the number from krs_abi_version() of the library it loaded. */
#define KRS_TYPE_F32 0
#define KRS_TYPE_C64 1
#define KRS_OUT_SAME 0
#define KRS_OUT_S16 1
#define KRS_MAX_L 1024
#define KRS_MAX_M 16384
#define KRS_MAX_RATIO 16 /* M <= 16 L */
#define KRS_MAX_PHASE_TAPS 256
#define KRS_MAX_TAPS 16384
#define KRS_MAX_IN 268435455 /* 2^28 - 1 */
#define KRS_MAX_POSITION 4503599627370496 /* 2^52 samples in */

typedef struct krs_resamp krs_resamp;

int krs_abi_version(void);
const char* krs_last_error(void);

/* A resampler on `device` with zero history and zero counts, its stream the NULL stream.  *out is NULL when refused. */
int krs_create(int32_t device, int32_t type, int32_t L, int32_t M, int32_t taps_per_phase, const float* taps_host,
               int32_t out_fmt, float pcm_scale, int64_t max_in, krs_resamp** out);
void krs_destroy(krs_resamp* h);

/* Work already enqueued on the old stream is ordered in front of work on the new one (an event is recorded on the OLD stream,
 * so a stream handed in here must stay alive until the next krs_set_stream / krs_destroy of this object). */
int krs_set_stream(krs_resamp* h, void* hip_stream);
int krs_synchronize(krs_resamp* h);

/* The number of outputs the next stream call of n_in samples yields: ceil((N0 + n_in) L / M) - ceil(N0 L / M). */
int krs_out_count(krs_resamp* h, int64_t n_in, int64_t* n_out);
/* The next n_in samples of the stream from device memory.  The outputs go to out_dev[0 .. *n_out) (float32, complex64 or
 * int16, out_capacity values), or with out_dev = NULL to the object's own buffer (out_capacity is ignored).  n_out may be
 * NULL.  Asynchronous. */
int krs_process_dev(krs_resamp* h, const void* in_dev, int64_t n_in, void* out_dev, int64_t out_capacity, int64_t* n_out);
/* The same from host memory into host memory (out_host [out_capacity] values); staged through library-owned device memory;
 * synchronises. */
int krs_process(krs_resamp* h, const void* in_host, int64_t n_in, void* out_host, int64_t out_capacity, int64_t* n_out);
/* The block form.  block_stride and block_len in samples, out_stride in output values.  Asynchronous. */
int krs_blocks_dev(krs_resamp* h, const void* in_dev, int64_t block_stride, int64_t nblocks, int64_t block_len, void* out_dev,
                   int64_t out_stride);

/* Replace the T taps (the same checks as krs_create); outputs already enqueued use the old taps, the history is kept.
 * Synchronises. */
int krs_set_taps(krs_resamp* h, const float* taps_host);
/* History to zero, counts to zero.  Asynchronous. */
int krs_reset(krs_resamp* h);
/* History to zero, counts as if samples_in zero samples had been fed, 0 .. 2^52.  Asynchronous. */
int krs_reset_at(krs_resamp* h, int64_t samples_in);
/* Samples in and samples out of the stream; any out pointer may be NULL.  No device work. */
int krs_state(krs_resamp* h, int64_t* samples_in, int64_t* samples_out);
/* The object's output buffer ([*capacity] values of float32, complex64 or int16), valid until krs_destroy: zero-copy for
 * torch.  capacity may be NULL. */
int krs_out_dev(krs_resamp* h, void** out_dev, int64_t* capacity);
/* Values [first, first + count) of the object's output buffer to out_host; synchronises. */
int krs_read_out(krs_resamp* h, void* out_host, int64_t first, int64_t count);

/* The filter kernel of the last launch (before any: of this object's plan, with a grid that fills the device): threads per
 * workgroup, LDS bytes per workgroup (static and dynamic), VGPRs, workgroups and outputs per workgroup.  The plan -- outputs
 * per workgroup and LDS bytes -- depends on (type, L, M, P) alone.  Any out pointer may be NULL. */
int krs_kernel_info(krs_resamp* h, int32_t* threads, int32_t* lds_bytes, int32_t* vgprs, int32_t* grid, int32_t* tile_out);

#ifdef __cplusplus
}
#endif

#endif
