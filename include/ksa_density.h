/* libksa_density -- C ABI of the spectrum density (persistence) histogram on the MI355X (gfx950): a companion of libksa.
 *
 * A density object is a bitmap of level against frequency: each cell counts how many spectra passed through that level at
 * that frequency.  It consumes the per-frame dB rows that libksa's entry points deliver in device memory (cur_db_dev of
 * ksa_frames_dev, out_dev of ksa_curscan_dev with KSA_OUT_DB) and nothing else of libksa: the two libraries share no symbol,
 * no state and no header.  The reference (hanishkvc/prgs-sdr-kspecanal) has no counterpart.
 *
 * Conventions are those of ksa.h: plain C types only; 0 = success, non-zero = error with text in ksd_last_error() (thread
 * local).  "host" pointers are ordinary CPU memory, "dev" pointers are HIP device memory of the object's device.  One object
 * = one GPU; no concurrent calls on one object.  All device work is enqueued on the object's stream (ksd_set_stream); entry
 * points that take or fill host memory synchronise that stream before returning, the others do not synchronise.  Every
 * entry point selects its object's device for its own duration and hands the caller's current HIP device back on return.
 * The library reads no environment variable.  A hipStream_t travels as void*.
 *
 * Semantics (the contract of every layer):
 *
 * A density object is created with:
 * - nbins: the row length, i.e. the engine's fft_size.
 * - width W: the number of bitmap columns.  It must divide nbins.  g = nbins / W bins fall into one column, as with hm_width.
 * - levels L and a level range [lo_db, hi_db).
 *
 * It owns int64 counts[L + 1][W] on the device, zero at creation, plus rows_seen.
 *
 * Adding a row r[0..nbins) of float32 dB values does the following for every bin b, all in float32:
 *
 *   inv  = (float)L / (hi_db - lo_db)    computed ONCE on the host at create time; one subtraction, one division
 *   t    = (r[b] - lo_db) * inv          one subtraction, then one multiplication; no fused or reassociated form
 *   row  = L                    if r[b] is NaN     (NaNs are counted in the extra last row and not in the bitmap)
 *          L - 1                if t >= (float)L   (+inf included)
 *          0                    if t < 0           (-inf included: an all-zero block's KSA_OUT_DB row lands in level 0)
 *          (int)t               otherwise          (truncation)
 *   counts[row][b / g] += 1
 *
 * Every (row, bin) pair adds exactly one count.  The invariant that follows: after any sequence of adds, every column of
 * counts sums to rows_seen * g.
 *
 * Counts are exact integers, so the result does not depend on grid size, chunking or arrival order.  No float atomics
 * anywhere.
 *
 * Limits, all refused by ksd_create with their own message and a null handle:
 * - 16 <= nbins <= 1048576
 * - 1 <= width, and nbins % width == 0
 * - 1 <= levels <= 1024
 * - lo_db and hi_db finite, lo_db < hi_db, and (float)L / (hi_db - lo_db) finite
 * - (levels + 1) * width <= 2^27, i.e. 1 GiB of counters
 *
 * Refused per call: null pointers, nrows < 0, row_stride < nbins, num / den outside their ranges.  A refused call leaves
 * counts and rows_seen as they were.
 */
#ifndef KSA_DENSITY_H
#define KSA_DENSITY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KSD_ABI_VERSION 1 /* A binding takes the number from ksd_abi_version() of the library it loaded. */
#define KSD_MIN_NBINS 16
#define KSD_MAX_NBINS 1048576
#define KSD_MAX_LEVELS 1024
#define KSD_MAX_CELLS 134217728 /* 2^27 cells of int64: (levels + 1) * width */

typedef struct ksd_density ksd_density;

int ksd_abi_version(void);
const char* ksd_last_error(void);

/* A zeroed histogram int64[levels + 1][width] on `device`, its stream the NULL stream.  *out is NULL when refused. */
int ksd_create(int32_t device, int32_t nbins, int32_t width, int32_t levels, float lo_db, float hi_db, ksd_density** out);
void ksd_destroy(ksd_density* d);

/* Same ordering rule as ksa_set_stream: work already enqueued on the old stream is ordered in front of work on the new one
 * (an event is recorded on the OLD stream, so a stream handed in here must stay alive until the next ksd_set_stream /
 * ksd_destroy of this object). */
int ksd_set_stream(ksd_density* d, void* hip_stream);
int ksd_synchronize(ksd_density* d);

/* Add nrows rows from device memory: row i is the nbins floats at rows_dev + i * row_stride (in floats, >= nbins).
 * Asynchronous on the object's stream, no synchronisation inside.  rows_dev is 4-byte aligned and nothing more is required
 * (16-byte loads are used when base and stride allow them).  nrows = 0 is a successful no-op. */
int ksd_add_rows_dev(ksd_density* d, const float* rows_dev, int64_t row_stride, int64_t nrows);
/* Add nrows contiguous rows (host[nrows][nbins]); staged through library-owned device memory; synchronises. */
int ksd_add_rows(ksd_density* d, const float* rows_host, int64_t nrows);

/* Every count (NaN row included) becomes floor(count * num / den), 0 <= num <= den, 1 <= den < 2^31, computed as
 * (c / den) * num + ((c % den) * num) / den so that no product leaves 64 bits.  rows_seen is left alone: what a display
 * calls between refreshes to fade old traces.  Asynchronous. */
int ksd_decay(ksd_density* d, int64_t num, int64_t den);
/* counts += counts_dev (int64[levels + 1][width] on the same device), rows_seen += rows_seen_add (>= 0): the multi-GPU
 * sum.  Asynchronous. */
int ksd_merge_dev(ksd_density* d, const int64_t* counts_dev, int64_t rows_seen_add);
/* Zero the counts and rows_seen.  Asynchronous. */
int ksd_reset(ksd_density* d);

/* Copy the counts to host int64[levels + 1][width] (counts_host may be NULL to fetch rows_seen alone) and return rows_seen
 * (rows_seen may be NULL); not both NULL.  Synchronises. */
int ksd_read(ksd_density* d, int64_t* counts_host, int64_t* rows_seen);
/* Device address of the counts, int64[levels + 1][width], valid until ksd_destroy: zero-copy for torch. */
int ksd_counts_dev(ksd_density* d, int64_t** counts_dev);

/* The add kernel chosen for this shape (the 16-byte-load form where the shape allows it): threads per workgroup, LDS bytes
 * per workgroup, VGPRs, workgroups of the last ksd_add_rows_dev launch (before any: of a launch that fills the device),
 * strip_cols = bitmap columns per workgroup, lds_optin = 1 when lds_bytes exceeds 64 KiB and the kernel's dynamic-LDS limit
 * was raised for it.  Any out pointer may be NULL. */
int ksd_kernel_info(ksd_density* d, int32_t* threads, int32_t* lds_bytes, int32_t* vgprs, int32_t* grid,
                    int32_t* strip_cols, int32_t* lds_optin);

#ifdef __cplusplus
}
#endif

#endif
