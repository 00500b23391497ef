/* libksa_pulse -- C ABI of the time-domain pulse detector and pulse list on the MI355X (gfx950): a companion of libksa.
 *
 * A pulse detector answers "when was something on the air" for a signal nobody has a template for (TDMA bursts, keyed
 * carriers, radar pulses, packet radio): it forms the power of raw IQ in device memory against time, smooths it over W samples,
 * compares it with a trigger level that has hysteresis, and lists the pulses it finds, each with its time of arrival, width,
 * energy, peak and the sum a carrier offset is read from (a pulse descriptor word).  It reads the raw samples the engine and
 * libksa_ddc read and nothing of either: it shares no symbol, no state and no header with libksa or the other companions.  The
 * reference (hanishkvc/prgs-sdr-kspecanal) has no counterpart.
 *
 * Conventions are those of the other headers: plain C types only; 0 = success, non-zero = error with text in
 * kpl_last_error() (thread local).  "host" pointers are ordinary CPU memory, "dev" pointers are HIP device memory of the
 * object's device (or page-locked mapped host memory).  One object = one GPU; no concurrent calls on one object.  All device
 * work is enqueued on the object's stream (kpl_set_stream); entry points that take or fill host memory synchronise that stream
 * before returning, the `_dev` ones do not synchronise.  Every entry point selects its object's device for its own duration
 * and hands the caller's current HIP device back on return.  The library reads no environment variable.  Argument checks come
 * before any HIP call.  A hipStream_t travels as void*.
 *
 * Semantics (the contract of every layer):
 *
 * The object is created with:
 * - device.
 * - fmt: the sample format, numbered and unpacked as in ksa_ddc.h.  KPL_FMT_C64 0: interleaved float32 I,Q.  KPL_FMT_U8 1:
 *   (float(byte) - u8_offset) * (1 / u8_scale), the reciprocal formed once in float32.  KPL_FMT_S8 2: float(int8) * 2^-7.
 *   KPL_FMT_S16 3: float(int16) * 2^-15.  Input pointers are aligned to the size of a sample (8, 2, 2, 4 bytes).
 * - W, 1 .. 4096: the length of the envelope's sliding sum.
 * - on_power, off_power: float32 linear mean powers, finite, 0 < off_power <= on_power <= 4.
 * - min_len, 1 .. 2^20: the shortest run that is a pulse.
 * - capacity, 1 .. 2^20 pulse records.
 * - max_in, 1 .. 2^28 - 1: the largest number of input samples per call (offsets inside one call are 32-bit; the start of a
 *   block, b * block_stride, and every position are formed in 64 bits).
 * Refused, each with its own text and a null handle: an unknown format, W, on_power, off_power, min_len, capacity or max_in
 * out of range, a thr_off (below) that comes out below 1, for KPL_FMT_U8 a u8_scale that is not finite and non-zero or a
 * u8_offset that is not finite, a negative device.
 *
 * Definition.  Every decision and every sum is an integer, so that no result can depend on tile, grid or how a stream is cut.
 * For sample n = (xr, xi) and its predecessor (yr, yi) = sample n-1, every operation an explicit round-to-nearest float32
 * operation and nothing contracted into a fused multiply-add:
 *
 *   p[n]  = fadd(fmul(xr, xr), fmul(xi, xi))
 *   q[n]  = (int64) rintf(fminf(p[n], 4.0f) * 2^30)          0 .. 2^32: power in units of 2^-30 of full scale, saturating at 4
 *   re[n] = fadd(fmul(xr, yr), fmul(xi, yi))                  x[n] conj(x[n-1])
 *   im[n] = fsub(fmul(xi, yr), fmul(xr, yi))
 *   dre[n], dim[n] = (int64) rintf(fminf(fmaxf(v, -4), 4) * 2^30)      of v = re[n], im[n]
 *
 * The product by 2^30 is exact and rintf rounds to nearest even; int8 and int16 input give q exactly.  Non-finite input gives
 * unspecified values and traps nowhere.
 *
 * Envelope: S[n] = q[n-W+1] + ... + q[n] in int64, q being 0 before the start of the stream or block; S < 2^45.
 *
 * Thresholds: the library forms, in float64, where both products are exact,
 *   thr_on  = llrint((double)on_power  * 2^30 * W),   thr_off = llrint((double)off_power * 2^30 * W)
 * and kpl_thresholds reports the two.  A thr_off below 1 is refused.
 *
 * Hysteresis: op[n] is SET if S[n] >= thr_on, CLEAR if S[n] < thr_off, else HOLD.  active[n] is the last op that is not HOLD at
 * or before n; it is 0 before the first one and 0 at the start of a stream or block.
 *
 * A pulse is a maximal run of active samples [start, start + len).  Runs shorter than min_len are dropped and counted nowhere.
 * A pulse is written as the 64 bytes of kpl_pulse below.
 *
 * - The buffer holds the FIRST `capacity` records since the last reset or clear, in ASCENDING (block, start) order, within a
 *   call and across calls.
 * - pulses_total counts every record, stored or not; active_total counts their samples.
 * - There are no float atomics anywhere (and no integer ones), and no result depends on the grid, on the tile or on how a
 *   stream is cut into calls.
 *
 * Stream form (kpl_process_dev, kpl_process, kpl_flush): one continuous stream cut into calls.  A call writes, where env is not
 * NULL, S of its n_in samples as int64 [n_in].  A run is recorded by the call that holds its first inactive sample, or by
 * kpl_flush, which closes the run still open at the end of the stream with KPL_FLAG_OPEN_END; after it the object refuses
 * stream calls until kpl_reset.  The object carries on the device the last W-1 values of q, the last unpacked sample, the
 * hysteresis state and the open run's partial record.  Dense output and records do not depend on how the stream is cut into
 * calls, bit for bit; n_in = 0 is a successful no-op.  Positions are int64; a call that would take samples_in past 2^52 is
 * refused.  `block` is -1 in the records of the stream form.
 *
 * Block form (kpl_blocks_dev): nblocks independent blocks.  Block b starts at iq_dev + b * block_stride samples (any
 * stride >= 0, blocks may overlap); nblocks * block_len <= max_in.  The stream state is neither read nor touched.  S of block b
 * goes to env_dev[b * out_stride + i].  A block gives, bit for bit, what a fresh stream of the same samples followed by
 * kpl_flush gives, with `block` = b.
 *
 * Refused per call, each with its own text and leaving the object as it was: a null object or required pointer, an input
 * pointer that is not aligned to the sample size, negative counts or strides, more than max_in samples, an out_stride below
 * block_len while env_dev is given, a stream call after kpl_flush, a stream position past 2^52.  A failure of the HIP runtime
 * inside a call is another matter: if a later launch of a stream call fails after its first, outputs and records may have been
 * written while the carried state has not moved consistently; the object then refuses further stream calls, with its own text,
 * until kpl_reset.  The block form keeps no such state.
 *
 * Work memory: the object owns S of max_in samples (int64) and a few words per tile of T samples (kpl_kernel_info) for
 * max_in / T + 1 tiles; a block-form call of many short blocks that needs more tiles than that enlarges the per-tile memory
 * once, after synchronising the stream.
 */
#ifndef KSA_PULSE_H
#define KSA_PULSE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KPL_ABI_VERSION 1 /* A binding takes the number from kpl_abi_version() of the library it loaded. */
#define KPL_FMT_C64 0
#define KPL_FMT_U8 1
#define KPL_FMT_S8 2
#define KPL_FMT_S16 3
#define KPL_MAX_W 4096
#define KPL_MAX_MIN_LEN 1048576
#define KPL_MAX_CAPACITY 1048576
#define KPL_MAX_IN 268435455 /* 2^28 - 1 */
#define KPL_MAX_POSITION 4503599627370496 /* 2^52 samples in */
#define KPL_POWER_UNIT 1073741824 /* 2^30: q, energy and S count full-scale power in units of 2^-30 */
#define KPL_FLAG_OPEN_END 1 /* the run was still active at the last sample of a flushed stream or of a block */

typedef struct kpl_detector kpl_detector;

/* One pulse.  The struct has no padding: 64 bytes in all, and `start` of record i lies at byte 64 i. */
#pragma pack(push, 4)
typedef struct kpl_pulse {
  int64_t start;    /* the first active sample: stream index, or index inside the block */
  int64_t len;      /* active samples */
  int64_t energy;   /* the sum of q over the run */
  int64_t peak;     /* the maximum of S over the run */
  int64_t peak_pos; /* the lowest n with that S */
  int64_t dre;      /* the sums of dre[n] and dim[n] over n = start+1 .. start+len-1: the pairs with both samples in the run */
  int64_t dim;
  int32_t block;    /* the block, -1 in the stream form */
  int32_t flags;    /* bit 0: KPL_FLAG_OPEN_END */
} kpl_pulse;
#pragma pack(pop)

int kpl_abi_version(void);
const char* kpl_last_error(void);

/* A detector on `device` with an empty stream and no record, its stream the NULL stream.  *out is NULL when refused. */
int kpl_create(int32_t device, int32_t fmt, float u8_offset, float u8_scale, int32_t W, float on_power, float off_power,
               int32_t min_len, int32_t capacity, int64_t max_in, kpl_detector** out);
void kpl_destroy(kpl_detector* h);

/* Work already enqueued on the old stream is ordered in front of work on the new one (an event is recorded on the OLD stream,
 * so a stream handed in here must stay alive until the next kpl_set_stream / kpl_destroy of this object). */
int kpl_set_stream(kpl_detector* h, void* hip_stream);
int kpl_synchronize(kpl_detector* h);

/* The next n_in samples of the stream from device memory.  env_dev (int64 [n_in], S) may be NULL.  Asynchronous. */
int kpl_process_dev(kpl_detector* h, const void* iq_dev, int64_t n_in, int64_t* env_dev);
/* The same from host memory into host memory; staged through library-owned device memory; synchronises. */
int kpl_process(kpl_detector* h, const void* iq_host, int64_t n_in, int64_t* env_host);
/* Close the run still open with KPL_FLAG_OPEN_END; the object refuses stream calls afterwards until kpl_reset.  Asynchronous. */
int kpl_flush(kpl_detector* h);
/* The block form.  block_stride, block_len and out_stride in samples; out_stride is only read when env_dev is not NULL.
 * Asynchronous. */
int kpl_blocks_dev(kpl_detector* h, const void* iq_dev, int64_t block_stride, int64_t nblocks, int64_t block_len, int64_t* env_dev,
                   int64_t out_stride);

/* Replace on_power and off_power (the same checks as kpl_create); work already enqueued uses the old values. */
int kpl_set_params(kpl_detector* h, float on_power, float off_power);
/* thr_on and thr_off as the library formed them; either out pointer may be NULL.  No device work. */
int kpl_thresholds(kpl_detector* h, int64_t* thr_on, int64_t* thr_off);
/* An empty stream, no record, both totals zero.  Asynchronous. */
int kpl_reset(kpl_detector* h);
/* Samples in, whether a run is open at the end of what the stream has taken (0 / 1) and the open run's start (-1 when none);
 * any out pointer may be NULL.  Synchronises when open or open_start is asked for. */
int kpl_state(kpl_detector* h, int64_t* samples_in, int32_t* open, int64_t* open_start);

/* Copy the first min(stored, max_records) pulse records to records_host (kpl_pulse[]; may be NULL to fetch the counts alone),
 * *stored = records in the buffer = min(total, capacity), *total = pulses_total, *active = active_total; any count pointer may
 * be NULL.  Synchronises. */
int kpl_read_events(kpl_detector* h, void* records_host, int64_t max_records, int64_t* stored, int64_t* total, int64_t* active);
/* Device addresses, valid until kpl_destroy: kpl_pulse[capacity] and int64 [2] = pulses_total, active_total (either out
 * pointer may be NULL, not both). */
int kpl_events_dev(kpl_detector* h, void** records_dev, int64_t** totals_dev);
/* Empty the record buffer and zero both totals; the stream state stays.  Asynchronous. */
int kpl_clear_events(kpl_detector* h);

/* The envelope kernel of the last launch (before any: with the grid of max_in samples): threads per workgroup, LDS bytes per
 * workgroup, VGPRs, workgroups and `tile`, the samples per workgroup T.  T is a constant and the LDS bytes depend on W alone.
 * Any out pointer may be NULL. */
int kpl_kernel_info(kpl_detector* h, int32_t* threads, int32_t* lds_bytes, int32_t* vgprs, int32_t* grid, int32_t* tile);

#ifdef __cplusplus
}
#endif

#endif
