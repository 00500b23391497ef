/* libksa_corr -- C ABI of the matched-filter correlator and peak list on the MI355X (gfx950): a companion of libksa.
 *
 * A correlator object answers "where in time is this known waveform": it slides Q templates of K complex samples (a sync word,
 * a preamble, a chirp, a bank of frequency-offset hypotheses of one of them) over raw IQ in device memory, forms for every lag
 * the correlation r and the normalised metric rho in [0, 1], and lists the lags at which rho peaks above a threshold, each with
 * its neighbours' metric (for a parabola) and its complex correlation (the carrier phase).  It reads the raw samples the
 * engine and libksa_ddc read and nothing of either: it shares no symbol, no state and no header with libksa or the other
 * companions.  The reference (hanishkvc/prgs-sdr-kspecanal) has no counterpart.
 *
 * Conventions are those of the other headers: plain C types only; 0 = success, non-zero = error with text in
 * kcr_last_error() (thread local).  "host" pointers are ordinary CPU memory, "dev" pointers are HIP device memory of the
 * object's device (or page-locked mapped host memory).  One object = one GPU; no concurrent calls on one object.  All device
 * work is enqueued on the object's stream (kcr_set_stream); entry points that take or fill host memory synchronise that stream
 * before returning, the `_dev` ones do not synchronise.  Every entry point selects its object's device for its own duration
 * and hands the caller's current HIP device back on return.  The library reads no environment variable.  Argument checks come
 * before any HIP call.  A hipStream_t travels as void*.
 *
 * Semantics (the contract of every layer):
 *
 * The object is created with:
 * - device.
 * - fmt: the sample format, numbered and unpacked as in ksa_ddc.h.  KCR_FMT_C64 0: interleaved float32 I,Q.  KCR_FMT_U8 1:
 *   (float(byte) - u8_offset) * (1 / u8_scale), the reciprocal formed once in float32.  KCR_FMT_S8 2: float(int8) * 2^-7.
 *   KCR_FMT_S16 3: float(int16) * 2^-15.  Input pointers are aligned to the size of a sample (8, 2, 2, 4 bytes).
 * - K, 1 .. 4096: the template length; Q, 1 .. 8: templates of that length, correlated against the same input in one pass; with
 *   Q K <= 16384.  templates_host is float32 [Q][K][2] (re, im).
 * - threshold: float32, finite, in (0, 1].  min_energy: float32, finite, >= 0.
 * - guard G, 1 .. 4096: the half width of the peak-picking neighbourhood.
 * - capacity, 1 .. 2^20 event records.
 * - max_in, 1 .. 2^28 - 1: the largest number of input samples per call (offsets inside one call are 32-bit; the start of a
 *   block, b * block_stride, and every position are formed in 64 bits).
 * Refused, each with its own text and a null handle: an unknown format, K, Q, Q K, threshold, min_energy, guard, capacity or
 * max_in out of range, null templates, a non-finite template value (the text names the template and the index), a template
 * whose energy is zero (or not finite), for KCR_FMT_U8 a u8_scale that is not finite and non-zero or a u8_offset that is not
 * finite, a negative device.
 *
 * The library forms Ec[q] = sum_k |c_q[k]|^2 in float64 and rounds it once to float32.
 *
 * The object owns on the device the templates, the stream's last K + 2 G - 1 unpacked samples, work buffers of rho and r for
 * Q (max_in + 2 G) lags, the event buffer of `capacity` records and an int64 events_total.  The host object holds the int64
 * counts of the stream.
 *
 * Definition.  Lag n is the stream (or block) index of the sample that meets c[0].  For template q, over k = 0 .. K-1
 * ascending, all in float32, every accumulator starting at +0:
 *
 *   re = fmaf(xr[n+k],  cr[k], re);   re = fmaf(xi[n+k], ci[k], re);
 *   im = fmaf(xr[n+k], -ci[k], im);   im = fmaf(xi[n+k], cr[k], im);
 *   e  = fmaf(xr[n+k], xr[n+k], e);   e  = fmaf(xi[n+k], xi[n+k], e);
 *
 * (re, im) is r_q[n] = sum_k conj(c_q[k]) x[n+k]; e is the energy of the window, shared by the Q templates.  Then
 *
 *   p = fmaf(re, re, im * im),   den = e * Ec[q],   rho_q[n] = (den > 0 && e >= min_energy) ? p / den : 0
 *
 * each operation rounded once, the division correctly rounded.  By Cauchy-Schwarz rho <= 1 up to rounding, and rho = 1 where
 * the window is a complex multiple of the template.  The order of every chain is a function of k alone, never of tile, grid
 * or call.  (Per k the real part's term comes before the imaginary part's: it is the order of a real matrix product over
 * k' = 2k, 2k+1.)  Non-finite input gives unspecified values and traps nowhere.
 *
 * Peaks.  Lag n is a peak of template q when rho_q[n] >= threshold, no existing lag j in [n-G, n) has rho_q[j] >= rho_q[n] and
 * no existing lag j in (n, n+G] has rho_q[j] > rho_q[n]: the lowest lag among equals wins.  Lags outside the stream or the
 * block do not exist and constrain nothing.  A peak is written as the 36 bytes of kcr_event below.
 *
 * - The buffer holds the FIRST `capacity` events since the last reset or clear, in ASCENDING (block, pos, templ) order, within
 *   a call and across calls.
 * - events_total counts every event, stored or not.
 * - There are no float atomics anywhere, and no result depends on the grid, on the tile or on how a stream is cut into calls.
 *
 * Stream form (kcr_process_dev, kcr_process, kcr_out_count, kcr_flush): one continuous stream cut into calls.  With N samples
 * in, lags 0 .. N-K exist.  A call that brings the total from N0 to N1 completes max(0, N1-K+1) - max(0, N0-K+1) lags
 * (kcr_out_count tells in advance) and writes, where the pointer is not NULL, rho of those lags to metric_dev[q * out_stride +
 * i] (float32) and r to corr_dev[q * out_stride + i] (complex64).  Lag n is decided once lag n+G exists; the call appends the
 * events of the lags it decides.  Dense outputs and events do not depend on how the stream is cut into calls, bit for bit;
 * n_in = 0 is a successful no-op.  The library keeps K + 2 G - 1 samples and recomputes the rho and r a decision needs.
 * kcr_flush decides the lags still pending at the end of a stream, their later neighbours taken as not existing; after it the
 * object refuses stream calls until kcr_reset.  Positions are int64; a call that would take samples_in past 2^52 is refused.
 * `block` is -1 in the events of the stream form.
 *
 * Block form (kcr_blocks_dev): nblocks independent blocks.  Block b starts at iq_dev + b * block_stride samples (any
 * stride >= 0, blocks may overlap); block_len >= K and nblocks * block_len <= max_in.  Lags 0 .. block_len-K exist in every
 * block, `pos` is counted inside the block and `block` = b.  The stream state is neither read nor touched.  Dense rows sit at
 * (b * Q + q) * out_stride + i.  A block cut out of a stream gives that stream's rho and r bit for bit at the same lags.
 *
 * Refused per call, each with its own text and leaving the object as it was: a null object or required pointer, an input
 * pointer that is not aligned to the sample size, negative counts or strides, more than max_in samples, block_len < K, an
 * out_stride below the lags of the call while a dense pointer is given, a stream call after kcr_flush, a stream position past
 * 2^52.  A failure of the HIP runtime inside a call is another matter: if a later launch of a stream call fails after its
 * first, outputs and events may have been written while history and counts have not moved; the object then refuses further
 * stream calls, with its own text, until kcr_reset.  The block form keeps no such state.
 */
#ifndef KSA_CORR_H
#define KSA_CORR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KCR_ABI_VERSION 1 /* A binding takes the number from kcr_abi_version() of the library it loaded. */
#define KCR_FMT_C64 0
#define KCR_FMT_U8 1
#define KCR_FMT_S8 2
#define KCR_FMT_S16 3
#define KCR_MAX_K 4096
#define KCR_MAX_Q 8
#define KCR_MAX_TEMPLATE_VALUES 16384 /* Q K */
#define KCR_MAX_GUARD 4096
#define KCR_MAX_CAPACITY 1048576
#define KCR_MAX_IN 268435455 /* 2^28 - 1 */
#define KCR_MAX_POSITION 4503599627370496 /* 2^52 samples in */

typedef struct kcr_corr kcr_corr;

/* One peak.  The struct has no padding: it is packed to 4 bytes, 36 bytes in all, and `pos` of record i lies at byte 36 i. */
#pragma pack(push, 4)
typedef struct kcr_event {
  int64_t pos;       /* the lag: stream index, or index inside the block */
  int32_t block;     /* the block, -1 in the stream form */
  int32_t templ;     /* q */
  float metric;      /* rho_q[pos] */
  float metric_prev; /* rho_q[pos-1], 0 where that lag does not exist */
  float metric_next; /* rho_q[pos+1], 0 where that lag does not exist */
  float re;          /* r_q[pos], bit for bit */
  float im;
} kcr_event;
#pragma pack(pop)

int kcr_abi_version(void);
const char* kcr_last_error(void);

/* A correlator on `device` with an empty stream and no event, its stream the NULL stream.  *out is NULL when refused. */
int kcr_create(int32_t device, int32_t fmt, float u8_offset, float u8_scale, int32_t K, int32_t Q, const float* templates_host,
               float threshold, float min_energy, int32_t guard, int32_t capacity, int64_t max_in, kcr_corr** out);
void kcr_destroy(kcr_corr* h);

/* Work already enqueued on the old stream is ordered in front of work on the new one (an event is recorded on the OLD stream,
 * so a stream handed in here must stay alive until the next kcr_set_stream / kcr_destroy of this object). */
int kcr_set_stream(kcr_corr* h, void* hip_stream);
int kcr_synchronize(kcr_corr* h);

/* The number of lags the next stream call of n_in samples completes. */
int kcr_out_count(kcr_corr* h, int64_t n_in, int64_t* n_lags);
/* The next n_in samples of the stream from device memory.  metric_dev (float32) and corr_dev (complex64) may each be NULL;
 * out_stride, in values, is only read when one of them is not.  n_lags may be NULL.  Asynchronous. */
int kcr_process_dev(kcr_corr* h, const void* iq_dev, int64_t n_in, float* metric_dev, void* corr_dev, int64_t out_stride,
                    int64_t* n_lags);
/* The same from host memory into host memory; staged through library-owned device memory; synchronises. */
int kcr_process(kcr_corr* h, const void* iq_host, int64_t n_in, float* metric_host, void* corr_host, int64_t out_stride,
                int64_t* n_lags);
/* Decide the lags still pending; the object refuses stream calls afterwards until kcr_reset.  Asynchronous. */
int kcr_flush(kcr_corr* h);
/* The block form.  block_stride and block_len in samples, out_stride in values.  Asynchronous. */
int kcr_blocks_dev(kcr_corr* h, const void* iq_dev, int64_t block_stride, int64_t nblocks, int64_t block_len, float* metric_dev,
                   void* corr_dev, int64_t out_stride);

/* Replace threshold and min_energy (the same checks as kcr_create); work already enqueued uses the old values. */
int kcr_set_params(kcr_corr* h, float threshold, float min_energy);
/* Replace the Q templates (the same checks as kcr_create); the stream state and the events are kept.  Synchronises. */
int kcr_set_templates(kcr_corr* h, const float* templates_host);
/* An empty stream, no event, events_total zero.  Asynchronous. */
int kcr_reset(kcr_corr* h);
/* Samples in, lags completed and lags decided of the stream; any out pointer may be NULL.  No device work. */
int kcr_state(kcr_corr* h, int64_t* samples_in, int64_t* lags_done, int64_t* lags_decided);

/* Copy the first min(stored, max_records) event records to records_host (kcr_event[]; may be NULL to fetch the two counts
 * alone), *stored = records in the buffer = min(total, capacity), *total = events_total; either count pointer may be NULL.
 * Synchronises. */
int kcr_read_events(kcr_corr* h, void* records_host, int64_t max_records, int64_t* stored, int64_t* total);
/* Device addresses, valid until kcr_destroy: kcr_event[capacity] and the int64 events_total (either out pointer may be NULL,
 * not both). */
int kcr_events_dev(kcr_corr* h, void** records_dev, int64_t** events_total_dev);
/* Empty the event buffer and zero events_total; the stream state stays.  Asynchronous. */
int kcr_clear_events(kcr_corr* h);

/* The correlation kernel of the last launch (before any: with a grid that fills the device): threads per workgroup, LDS bytes
 * per workgroup, VGPRs, workgroups and lags per workgroup (W).  W depends on Q alone and the LDS bytes on (K, Q) alone.  Any out
 * pointer may be NULL. */
int kcr_kernel_info(kcr_corr* h, int32_t* threads, int32_t* lds_bytes, int32_t* vgprs, int32_t* grid, int32_t* tile_out);

#ifdef __cplusplus
}
#endif

#endif
