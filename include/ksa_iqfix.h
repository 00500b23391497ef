/* libksa_iqfix -- C ABI of the DC-offset and IQ-imbalance corrector on the MI355X (gfx950): a companion of libksa.
 *
 * A direct-conversion receiver leaves two artefacts in its IQ: a DC offset (the spike in the centre bin) and a gain and phase
 * error between I and Q (which mirrors every signal at -f, some 20 to 30 dB down).  This library conditions raw IQ in device
 * memory in one pass: it applies a correction and writes complex64, and it accumulates the five integer sums the correction is
 * estimated from.  A host-side solve turns the sums into the correction.  It sits in front of the engine and of every other
 * companion and shares no symbol, no state and no header with any of them.  The reference (hanishkvc/prgs-sdr-kspecanal) has
 * no counterpart.
 *
 * Conventions are those of the other headers: plain C types only; 0 = success, non-zero = error with text in
 * kqf_last_error() (thread local).  "host" pointers are ordinary CPU memory, "dev" pointers are HIP device memory of the
 * object's device (or page-locked mapped host memory).  One object = one GPU; no concurrent calls on one object.  All device
 * work is enqueued on the object's stream (kqf_set_stream); entry points that take or fill host memory synchronise that stream
 * before returning, the `_dev` ones do not synchronise.  Every entry point selects its object's device for its own duration
 * and hands the caller's current HIP device back on return.  The library reads no environment variable.  Argument checks come
 * before any HIP call.  A hipStream_t travels as void*.
 *
 * Semantics (the contract of every layer):
 *
 * The object is created with:
 * - device.
 * - fmt: the sample format, numbered and unpacked as in ksa_ddc.h.  KQF_FMT_C64 0: interleaved float32 I,Q.  KQF_FMT_U8 1:
 *   (float(byte) - u8_offset) * (1 / u8_scale), the reciprocal formed once in float32.  KQF_FMT_S8 2: float(int8) * 2^-7.
 *   KQF_FMT_S16 3: float(int16) * 2^-15.  Input pointers are aligned to the size of a sample (8, 2, 2, 4 bytes).
 * - max_in, 1 .. 2^28 - 1: the largest number of input samples per call (offsets inside one block are 32-bit; the start of a
 *   block, b * block_stride, is formed in 64 bits).
 * Refused, each with its own text and a null handle: an unknown format, max_in out of range, for KQF_FMT_U8 a u8_scale that is
 * not finite and non-zero or a u8_offset that is not finite, a negative device.
 * The object starts with the identity coefficients (dc_i, dc_q, c, d) = (0, 0, 0, 1), zero sums and the NULL stream.
 *
 * The operation has no memory from sample to sample: there is no stream state, and the flat form is the block form with
 * nblocks = 1.
 *
 * Statistics.  For each unpacked raw sample (xr, xi) five integers are formed, every operation an explicit round-to-nearest
 * float32 operation and nothing contracted into a fused multiply-add:
 *
 *   aI  = (int64) rintf(fmaxf(fminf(xr, 4), -4) * 2^30)            aQ likewise of xi
 *   cII = (int64) rintf(fminf(fmul(xr, xr), 4) * 2^30)             cQQ likewise of xi
 *   cIQ = (int64) rintf(fmaxf(fminf(fmul(xr, xi), 4), -4) * 2^30)
 *
 * Each is at most 2^32 in magnitude; the product by 2^30 is exact and rintf rounds ties to even.  Non-finite input gives
 * unspecified values and traps nowhere.  The object holds int64 sums[6] = sum aI, sum aQ, sum cII, sum cQQ, sum cIQ, count on
 * the device, and the host keeps its own copy of count.  A call that would take count past KQF_MAX_COUNT = 2^30 is refused
 * before any launch and changes nothing, so every sum stays below 2^62.  The sums are integers: they do not depend on grid,
 * tile or how the input is cut into calls.  There are no float atomics anywhere (and no integer ones): workgroups leave
 * partial sums and a small finishing kernel adds them.
 *
 * Solve (kqf_solve): synchronises, reads the six words and computes in float64 on the host, every operation rounded on its
 * own (nothing contracted), so that the same lines in any IEEE float64 arithmetic give the same bits:
 *
 *   u = (double)count * 2^30
 *   mI = (double)sum aI / u          mQ = (double)sum aQ / u
 *   vII = (double)sum cII / u - mI mI      vQQ = (double)sum cQQ / u - mQ mQ      vIQ = (double)sum cIQ / u - mI mQ
 *   dc_i, dc_q = (float)mI, (float)mQ  with KQF_MODE_DC, else 0, 0
 *   with KQF_MODE_IQ:  r = vIQ / vII,  w = vQQ - r vIQ,  d = sqrt(vII / w),  c = -(d r),  both then rounded to float32;
 *     valid only if vII > 0 and w > 0 and 2^-8 <= vII / w <= 2^8, otherwise c = 0, d = 1 and KQF_FLAG_DEGENERATE is set
 *   without KQF_MODE_IQ:  c = 0, d = 1
 *
 * This is Gram-Schmidt: after it the corrected I and Q of the measured data are zero-mean, uncorrelated and of equal power.
 * mode is KQF_MODE_DC | KQF_MODE_IQ; 0 or any other bit is refused.  count == 0 gives the identity coefficients and
 * KQF_FLAG_EMPTY, and the call succeeds.  The result becomes the object's coefficients for every later call; work already
 * enqueued keeps the old ones, because coefficients travel as kernel arguments.
 *
 * Apply.  Four explicit float32 operations per sample:
 *
 *   uI = fsub(xr, dc_i)      uQ = fsub(xi, dc_q)      yI = uI      yQ = fadd(fmul(c, uI), fmul(d, uQ))
 *
 * Output is interleaved float32 I,Q.  The identity coefficients give the unpacked input as values (a -0 may come out as +0).
 *
 * Block form (kqf_blocks_dev): block b starts at iq_dev + b * block_stride samples (any stride >= 0, blocks may overlap);
 * nblocks * block_len <= max_in.  Output sample i of block b goes to out_dev[b * out_stride + i] with out_stride >= block_len;
 * nothing between blocks or past the last one is written.  out_dev NULL means the library's own packed buffer of max_in
 * complex64 (out_stride is then not read; kqf_out_dev gives its address; it is allocated when first needed).  With
 * accumulate != 0 the raw samples of the call also enter the sums in the same pass: the input is read once, and a sample that
 * lies in two overlapping blocks counts twice.  For KQF_FMT_C64, out_dev == iq_dev with out_stride == block_stride >= block_len
 * works in place; any other overlap of input and output is undefined.  nblocks = 0 or block_len = 0 is a successful no-op.
 *
 * Refused per call, each with its own text and leaving the object as it was: a null object or required pointer, an input
 * pointer that is not aligned to the sample size, an out_dev that is not aligned to 8 bytes, negative counts or strides, more
 * than max_in samples, an out_stride below block_len while out_dev is given, a count past 2^30, non-finite coefficients, a bad
 * mode.
 */
#ifndef KSA_IQFIX_H
#define KSA_IQFIX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KQF_ABI_VERSION 1 /* A binding takes the number from kqf_abi_version() of the library it loaded. */
#define KQF_FMT_C64 0
#define KQF_FMT_U8 1
#define KQF_FMT_S8 2
#define KQF_FMT_S16 3
#define KQF_MAX_IN 268435455 /* 2^28 - 1 */
#define KQF_MAX_COUNT 1073741824 /* 2^30 samples in the sums */
#define KQF_UNIT 1073741824 /* 2^30: the sums count full scale in units of 2^-30 */
#define KQF_MODE_DC 1
#define KQF_MODE_IQ 2
#define KQF_FLAG_DEGENERATE 1 /* KQF_MODE_IQ was asked for and the sums do not determine c and d: c = 0, d = 1 */
#define KQF_FLAG_EMPTY 2 /* count was 0: the identity coefficients */

typedef struct kqf_corrector kqf_corrector;

/* The coefficients and what the solve that made them saw.  The struct has no padding: 32 bytes in all. */
typedef struct kqf_coeffs {
  float dc_i, dc_q, c, d;
  int32_t flags, mode; /* of the last kqf_solve; 0, 0 at the start and after kqf_set_coeffs */
  int64_t count;       /* samples in the sums that solve read; 0 at the start and after kqf_set_coeffs */
} kqf_coeffs;

int kqf_abi_version(void);
const char* kqf_last_error(void);

/* A corrector on `device` with identity coefficients and zero sums, its stream the NULL stream.  *out is NULL when refused. */
int kqf_create(int32_t device, int32_t fmt, float u8_offset, float u8_scale, int64_t max_in, kqf_corrector** out);
void kqf_destroy(kqf_corrector* h);

/* Work already enqueued on the old stream is ordered in front of work on the new one (an event is recorded on the OLD stream,
 * so a stream handed in here must stay alive until the next kqf_set_stream / kqf_destroy of this object). */
int kqf_set_stream(kqf_corrector* h, void* hip_stream);
int kqf_synchronize(kqf_corrector* h);

/* The block form: correct, and with accumulate != 0 also take the raw samples into the sums.  block_stride, block_len and
 * out_stride in samples; out_stride is only read when out_dev is not NULL.  Asynchronous. */
int kqf_blocks_dev(kqf_corrector* h, const void* iq_dev, int64_t block_stride, int64_t nblocks, int64_t block_len, void* out_dev,
                   int64_t out_stride, int32_t accumulate);
/* The sums alone: nothing is written but the sums.  Asynchronous. */
int kqf_accumulate_dev(kqf_corrector* h, const void* iq_dev, int64_t block_stride, int64_t nblocks, int64_t block_len);
/* One block of n samples from host memory to out_host (complex64 [n]); staged through library-owned device memory;
 * synchronises.  out_host may be NULL when accumulate != 0: the sums alone. */
int kqf_apply(kqf_corrector* h, const void* iq_host, int64_t n, void* out_host, int32_t accumulate);

/* Sums -> coefficients (above); they become the object's.  *out may be NULL.  Synchronises. */
int kqf_solve(kqf_corrector* h, int32_t mode, kqf_coeffs* out);
/* Four finite values; they hold from the next call.  No device work. */
int kqf_set_coeffs(kqf_corrector* h, float dc_i, float dc_q, float c, float d);
/* The object's coefficients.  No device work. */
int kqf_get_coeffs(kqf_corrector* h, kqf_coeffs* out);

/* The six words sum aI, sum aQ, sum cII, sum cQQ, sum cIQ, count.  Synchronises. */
int kqf_read_stats(kqf_corrector* h, int64_t sums[6]);
/* Their device address, valid until kqf_destroy. */
int kqf_stats_dev(kqf_corrector* h, int64_t** sums_dev);
/* Zero the six words; the host's count is zero at once.  Asynchronous. */
int kqf_clear_stats(kqf_corrector* h);
/* The device address of the library's own output buffer, complex64 [max_in], valid until kqf_destroy. */
int kqf_out_dev(kqf_corrector* h, void** out_dev);

/* The kernel of the last launch (before any: the apply-only one with the grid of max_in samples): threads per workgroup, LDS
 * bytes per workgroup, VGPRs, workgroups and `tile`, the samples a workgroup takes at a time, a constant.  Any out pointer may
 * be NULL. */
int kqf_kernel_info(kqf_corrector* h, int32_t* threads, int32_t* lds_bytes, int32_t* vgprs, int32_t* grid, int32_t* tile);

#ifdef __cplusplus
}
#endif

#endif
