/* libksa_chan -- C ABI of the polyphase channelizer on the MI355X (gfx950): a companion of libksa.
 *
 * A channelizer object turns one wideband IQ stream into all M of its equally spaced channels at once, every channel shifted
 * to 0 Hz, low-pass filtered by one prototype and decimated by D = M / O.  M down-converter objects (ksa_ddc.h) over the same
 * input compute the same thing at M reads of the capture and M * T / D multiply-adds per sample; the polyphase structure costs
 * T / D and one M-point transform for all channels together.  The result is channel-major: every channel is a contiguous
 * complex64 time series in device memory, which is what kdm_blocks_dev (nblocks = M, block_stride = chan_stride) and
 * ksa_frames_dev already accept.  It shares no symbol, no state and no header with libksa or the other companions.  The
 * reference (hanishkvc/prgs-sdr-kspecanal) has no counterpart.
 *
 * Conventions are those of ksa_ddc.h: plain C types only; 0 = success, non-zero = error with text in kch_last_error() (thread
 * local).  "host" pointers are ordinary CPU memory, "dev" pointers are HIP device memory of the object's device (or page-locked
 * mapped host memory).  One object = one GPU; no concurrent calls on one object.  All device work is enqueued on the object's
 * stream (kch_set_stream); entry points that take or fill host memory synchronise that stream before returning, the `_dev`
 * ones do not synchronise.  Every entry point selects its object's device for its own duration and hands the caller's current
 * HIP device back on return.  The library reads no environment variable.  Argument checks come before any HIP call.  A
 * hipStream_t travels as void*.  There are no float atomics, and no result depends on grid or tile.
 *
 * Semantics (the contract of every layer):
 *
 * Object.  kch_create(device, fmt, u8_offset, u8_scale, nchan M, oversample O, taps_per_branch P, taps_host float32[M * P],
 * max_in, &h):
 * - fmt: the sample format of the input, interleaved I,Q, little-endian, with the values and unpack rules of ksa_ddc.h:
 *     KCH_FMT_C64 = 0  float32 pairs, 8 bytes per sample, taken as they are
 *     KCH_FMT_U8  = 1  uint8 pairs, 2 bytes per sample, (b - u8_offset) * (1 / u8_scale); 1 / u8_scale is rounded to float32 once
 *     KCH_FMT_S8  = 2  int8 pairs, 2 bytes per sample, b / 128
 *     KCH_FMT_S16 = 3  int16 pairs, 4 bytes per sample, b / 32768
 *   u8_offset and u8_scale are only read for KCH_FMT_U8.  An input pointer is aligned to its sample size (8, 2, 2, 4 bytes).
 * - M, the number of channels: a power of two, 2 .. 1024.
 * - O, the oversampling: 1, 2 or 4, with D = M / O >= 1 the decimation (input samples per output column).
 * - P, the taps per branch: 1 .. 32, with T = M * P <= 8192 the length of the real prototype h.
 * - max_in: the largest number of input samples per call, 1 .. 2^28 - 1 (offsets inside one call are 32-bit; the start of a
 *   block, b * block_stride, is formed in 64 bits).
 * Refused, each with its own text and a null handle: M, O, D, P, T or max_in out of range, null taps, a non-finite tap, an
 * unknown format, a zero or non-finite u8_scale or a non-finite u8_offset (KCH_FMT_U8), a negative device.
 *
 * Definition.  Channel c, 0 <= c < M, is centred at c / M cycles per input sample, so c >= M / 2 are the negative frequencies:
 *   y[c][m] = sum_{k<T} h[k] * x[m*D - k] * exp(-2 pi i c (m*D - k) / M),   x[n] = 0 for n < 0
 * This is what a kdc_ down-converter with phase_inc = c * 2^64 / M, decim = D and the same taps computes.
 *
 * Evaluation.  With k = p + M q:
 *   u_m[p] = sum_{q<P} h[p + M q] * x[m*D - p - M q]     one float32 chain of fused multiply-adds per part, q ascending
 *   z_m[c] = sum_{p<M} u_m[p] * exp(+2 pi i c p / M)      an M-point transform whose network depends on M alone
 *   y[c][m] = z_m[c] * exp(-2 pi i c m / O)               exactly 1, (-1)^(c m) or (-i)^(c m): signs and swaps, no multiply
 * The transform is the radix-2 decimation-in-time network on bit-reversed u (its stages run two at a time; the arithmetic is
 * that of the radix-2 network).  A butterfly is a' = a + w b, b' = a - w b with w b = (wr br - wi bi, wr bi + wi br), each part
 * one multiply and one fused multiply-add.  The twiddle factors come from a table built on the host in float64 and rounded
 * once to float32; they are exact on the axes, (1,0) and (0,1), so channels 0, M/4, M/2 and 3M/4 of integer data are exact.
 * Because chain order and network are functions of (M, O, P) alone, the same column gives the same bits however a stream is
 * cut, whichever tile it falls in, and in either form.
 *
 * Stream form (kch_process_dev, kch_process): one continuous stream cut into calls.  Column m exists once input m*D has
 * arrived: a call that takes the total from N0 to N1 samples yields ceil(N1 / D) - ceil(N0 / D) columns (kch_out_count tells
 * in advance); n_in = 0 is a successful no-op.  Column j of the call for channel c goes to out_dev[c * chan_stride + j]
 * (complex64, chan_stride >= n_out, in values); out_dev = NULL writes the object's own buffer at
 * chan_stride = ceil(max_in / D) + 1.  The object keeps T - 1 unpacked history samples on the device, in two buffers, with a
 * history kernel after the filter kernel; the host keeps the counts, and the column index mod O follows from samples_out.  If
 * the second launch of a call (the history) fails after the first (the filter), outputs may have been written while history
 * and counts have not moved; the object then refuses further stream calls, with its own text, until kch_reset.
 *
 * Block form (kch_blocks_dev): nblocks independent captures, block b at iq_dev + b * block_stride samples (any stride >= 0,
 * blocks may overlap).  It is the stream form run on each block alone with the start-up transient dropped: with
 * first = ceil((T - 1) / D) (= O * P for D > 1, T - 1 for D = 1),
 *   out[b][c][j] = y_b[c][first + j],   j < J = (block_len - 1) / D - first + 1
 * Refused unless block_len >= first * D + 1 and nblocks * block_len <= max_in.  Output b, c, j goes to
 * out_dev[(b * M + c) * chan_stride + j] (chan_stride >= J); out_dev = NULL writes the object's own buffer at chan_stride = J.
 * block_len = D * (first + F - 1) + 1 gives exactly F columns.  The stream state is neither read nor touched.  Block and stream
 * agree bit for bit.  n counts from the block's first sample (the mixer restarts in every block): a block that starts s samples
 * into a stream gives that stream's columns times exp(-2 pi i c s / M), which is 1 where s is a multiple of M.
 *
 * All objects of one format run one kernel function, whose dynamic-LDS limit the library sets once to 160 KiB, the most any
 * plan may ask for: objects of different shapes do not disturb each other.
 *
 * The object's own buffer holds M * (ceil(max_in / D) + 1) complex64 values, which is room for any permitted call.  It is read
 * as rows: the last call that wrote it left `rows` rows (M in the stream form, nblocks * M in the block form, row b * M + c)
 * at a row stride (kch_out_dev reports both); before any call that is M rows at ceil(max_in / D) + 1.
 *
 * Level meter (kch_channel_power): per channel c the sum of re^2 + im^2 over values [first, first + count) of every row of
 * channel c in the object's own buffer (one row in the stream form, one per block in the block form, blocks in order).
 * Products and sums are float64 in a fixed order: one workgroup of 256 threads per channel, thread t takes the values
 * first + t, first + t + 256, .. of every row, rows in order, and the 256 partial sums meet in a fixed tree (128, 64, .. 1).
 * Synchronises.
 *
 * Refused per call, each with its own text and leaving the object as it was: a null object, a null input pointer (with n > 0),
 * a misaligned input pointer, a negative count, more than max_in samples, a short block, a negative stride, chan_stride too
 * small, a row or range out of bounds in kch_read_out / kch_channel_power.
 */
#ifndef KSA_CHAN_H
#define KSA_CHAN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KCH_ABI_VERSION 1 /* A binding takes the number from kch_abi_version() of the library it loaded. */
#define KCH_FMT_C64 0
#define KCH_FMT_U8 1
#define KCH_FMT_S8 2
#define KCH_FMT_S16 3
#define KCH_MIN_CHAN 2
#define KCH_MAX_CHAN 1024
#define KCH_MAX_BRANCH_TAPS 32
#define KCH_MAX_TAPS 8192
#define KCH_MAX_IN 268435455 /* 2^28 - 1 */
/* kernel form reported by kch_kernel_info */
#define KCH_FORM_LDS 0 /* the tile's span and its W transforms in LDS, two radix-2 stages per pass */

typedef struct kch_chan kch_chan;

int kch_abi_version(void);
const char* kch_last_error(void);

/* A channelizer on `device` with zero history and zero counts, its stream the NULL stream.  *out is NULL when refused. */
int kch_create(int32_t device, int32_t fmt, float u8_offset, float u8_scale, int32_t nchan, int32_t oversample,
               int32_t taps_per_branch, const float* taps_host, int64_t max_in, kch_chan** out);
void kch_destroy(kch_chan* h);

/* Work already enqueued on the old stream is ordered in front of work on the new one (an event is recorded on the OLD stream,
 * so a stream handed in here must stay alive until the next kch_set_stream / kch_destroy of this object). */
int kch_set_stream(kch_chan* h, void* hip_stream);
int kch_synchronize(kch_chan* h);

/* The number of columns the next stream call of n_in samples yields: ceil((N0 + n_in) / D) - ceil(N0 / D). */
int kch_out_count(kch_chan* h, int64_t n_in, int64_t* n_out);
/* The next n_in samples of the stream from device memory.  n_out may be NULL; it is written only when the call succeeds.
 * Asynchronous. */
int kch_process_dev(kch_chan* h, const void* iq_dev, int64_t n_in, void* out_dev, int64_t chan_stride, int64_t* n_out);
/* The same from host memory into host memory (out_host complex64, channel c at c * chan_stride); staged through library-owned
 * device memory and the object's own buffer; synchronises. */
int kch_process(kch_chan* h, const void* iq_host, int64_t n_in, void* out_host, int64_t chan_stride, int64_t* n_out);
/* The block form.  block_stride and block_len in samples, chan_stride in complex64 values.  Asynchronous. */
int kch_blocks_dev(kch_chan* h, const void* iq_dev, int64_t block_stride, int64_t nblocks, int64_t block_len, void* out_dev,
                   int64_t chan_stride);
/* power_host float64[M]; see "Level meter".  Synchronises. */
int kch_channel_power(kch_chan* h, int64_t first, int64_t count, double* power_host);

/* Replace the M * P taps (the same checks as kch_create); outputs already enqueued use the old taps, the history is kept.
 * Synchronises. */
int kch_set_taps(kch_chan* h, const float* taps_host);
/* History and counts to zero.  Asynchronous. */
int kch_reset(kch_chan* h);
/* Samples in and columns out of the stream; any out pointer may be NULL.  No device work. */
int kch_state(kch_chan* h, int64_t* samples_in, int64_t* samples_out);
/* The object's own buffer (complex64), valid until kch_destroy: zero-copy for torch.  rows and row_stride describe what the
 * last call left there; capacity is the buffer's size in values.  Any of the last three may be NULL. */
int kch_out_dev(kch_chan* h, void** out_dev, int64_t* rows, int64_t* row_stride, int64_t* capacity);
/* Values [first, first + count) of row `chan` of the object's own buffer to out_host (complex64[count]).  Synchronises. */
int kch_read_out(kch_chan* h, void* out_host, int64_t chan, int64_t first, int64_t count);

/* The main kernel of the last launch (before any: with a grid that fills the device): threads per workgroup, LDS bytes per
 * workgroup, VGPRs, workgroups, columns per workgroup W, and form = KCH_FORM_LDS.  The plan (threads, LDS, W, form) is a
 * function of (M, O, P) alone.  Any out pointer may be NULL. */
int kch_kernel_info(kch_chan* h, int32_t* threads, int32_t* lds_bytes, int32_t* vgprs, int32_t* grid, int32_t* tile_cols,
                    int32_t* form);

#ifdef __cplusplus
}
#endif

#endif
