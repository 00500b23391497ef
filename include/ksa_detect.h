/* libksa_detect -- C ABI of the CFAR signal detector and emission list on the MI355X (gfx950): a companion of libksa.
 *
 * A detector object estimates, for every bin of every spectrum, the local noise floor from the bins around it (CFAR: constant
 * false-alarm rate), thresholds the bin against that floor, groups the detected bins of a row into emissions (start bin, stop
 * bin, peak, floor) and counts, per bin, the rows in which the bin lay inside an emission.  It consumes the per-frame dB rows
 * that libksa's entry points deliver in device memory (cur_db_dev of ksa_frames_dev, out_dev of ksa_curscan_dev with
 * KSA_OUT_DB) and nothing else of libksa: the libraries share no symbol, no state and no header.  The reference
 * (hanishkvc/prgs-sdr-kspecanal) has no counterpart: its marker list (ksa_read_highs here) knows no floor and no width.
 *
 * Conventions are those of ksa_mask.h: plain C types only; 0 = success, non-zero = error with text in kse_last_error()
 * (thread local).  "host" pointers are ordinary CPU memory, "dev" pointers are HIP device memory of the object's device.  One
 * object = one GPU; no concurrent calls on one object.  All device work is enqueued on the object's stream (kse_set_stream);
 * entry points that take or fill host memory synchronise that stream before returning, the others do not synchronise.  Every
 * entry point selects its object's device for its own duration and hands the caller's current HIP device back on return.  The
 * library reads no environment variable.  Argument checks come before any HIP call.  A hipStream_t travels as void*.
 *
 * Semantics (the contract of every layer).  Every decision is an integer, so the results never depend on grid, chunking or
 * arrival order.
 *
 * A detector object is created with:
 * - nbins, 16 .. 16384, any value: the row length, i.e. the engine's fft_size (one row lives in one workgroup's LDS).
 * - train, 1 .. 1024: training cells on either side.
 * - guard, 0 .. 256: guard cells on either side.
 * - threshold_db, float32, finite, 0 .. 100.
 * - mode: KSE_MODE_CA 0 (cell averaging), KSE_MODE_GO 1 (greatest of), KSE_MODE_SO 2 (smallest of).
 * - min_width, 1 .. nbins.
 * - max_gap, 0 .. 1024.
 * - capacity, 1 .. 2^20 emission records.
 * - device >= 0.
 * Each out-of-range parameter is refused with its own text and a null handle.
 *
 * The object owns on the device int64 hits[nbins] (zero at creation), an emission buffer of `capacity` records and an int64
 * emissions_total.  The host object holds rows_seen, which is also the index the next row gets; kse_set_row_base overwrites
 * it.
 *
 * Quantise.  For bin b of a row r, x = r[b] in float32:
 *
 *   valid = !(x != x) && x != -inf
 *   q     = (int32) rintf(fminf(fmaxf(x, -500), 500) * 64)      for valid x
 *
 * The unit is 1/64 dB, rounding is to nearest even, the product by 64 is exact; +inf becomes 32000.  Invalid bins contribute
 * nothing to any sum, are never detected and are never a peak.
 *
 * Noise estimate.  The lagging cells of bin b are bins b-guard-train .. b-guard-1, the leading cells b+guard+1 ..
 * b+guard+train, both clipped to [0, nbins): there is no wrap-around.  SL, CL = the sum of q and the count of the valid
 * cells on the lagging side, SR, CR the same on the leading side.
 *
 *   tq         = (int32) rintf(threshold_db * 64)
 *   pass(S, C) = C > 0 && q*C > S + tq*C                         in int32 (no magnitude exceeds 2^27)
 *
 * Raw detection det0[b] = valid and
 * - CA: pass(SL+SR, CL+CR);
 * - GO: pass against every side that has C > 0, and at least one side has ("greater than the greater mean" without a
 *   division);
 * - SO: pass against at least one side.
 * A bin with no valid training cell on either side is never detected.
 *
 * Grouping.
 * 1. Opening: keep[b] = det0[b] and b lies in a run of consecutive det0 bins at least min_width long.
 * 2. Closing: a gap of at most max_gap non-keep bins with a keep bin on each side is bridged.
 * 3. An emission is a maximal run of kept-or-bridged bins, [bin_lo, bin_hi] inclusive; both ends are keep bins.
 *
 * Record: the 32 bytes of kse_emission below.  `row` is the running index: rows_seen before the call plus the row's position
 * in the call.  peak_bin is the keep bin with the largest q, the lowest bin among equals; ndet the number of keep bins in the
 * run; peak_db the row's own float32 at peak_bin, bit for bit; floor_db the estimate at peak_bin:
 *
 *   floor_db = (float)S / (float)C * 2^-6      two int32 -> float32 conversions, one correctly rounded float32 division
 *
 * with S, C the pooled SL+SR, CL+CR for CA, the side with the greater mean for GO and the side with the smaller mean for SO.
 * The side is decided by SL*CR against SR*CL in int64, a tie going to the lagging side; a side with C = 0 is no candidate.
 *
 * - The buffer holds the FIRST `capacity` emissions since the last reset or clear, in ASCENDING (row, bin_lo) order, within a
 *   call and across calls.
 * - emissions_total counts every emission, stored or not.
 * - hits[b] gains 1 for every bin in [bin_lo, bin_hi] of every emission, stored or not; divided by rows_seen it is the
 *   occupancy against the adaptive threshold.
 * - There are no float atomics anywhere.
 *
 * Refused per call, leaving everything as it was: null required pointers, nrows < 0, row_stride < nbins, max_records < 0,
 * a negative row base, a negative rows_seen_add.
 */
#ifndef KSA_DETECT_H
#define KSA_DETECT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KSE_ABI_VERSION 1 /* A binding takes the number from kse_abi_version() of the library it loaded. */
#define KSE_MIN_NBINS 16
#define KSE_MAX_NBINS 16384
#define KSE_MAX_TRAIN 1024
#define KSE_MAX_GUARD 256
#define KSE_MAX_GAP 1024
#define KSE_MAX_CAPACITY 1048576
#define KSE_MODE_CA 0
#define KSE_MODE_GO 1
#define KSE_MODE_SO 2

typedef struct kse_detector kse_detector;

typedef struct kse_emission {
  int64_t row;      /* running row index */
  int32_t bin_lo;   /* first bin of the emission, a keep bin */
  int32_t bin_hi;   /* last bin of the emission (inclusive), a keep bin */
  int32_t peak_bin; /* the keep bin with the largest q, the lowest among equals */
  int32_t ndet;     /* keep bins in [bin_lo, bin_hi] */
  float peak_db;    /* the row's float32 at peak_bin */
  float floor_db;   /* the noise estimate at peak_bin */
} kse_emission;

int kse_abi_version(void);
const char* kse_last_error(void);

/* A detector object on `device` with zeroed hits and no emission, its stream the NULL stream.  *out is NULL when refused. */
int kse_create(int32_t device, int32_t nbins, int32_t train, int32_t guard, float threshold_db, int32_t mode,
               int32_t min_width, int32_t max_gap, int32_t capacity, kse_detector** out);
void kse_destroy(kse_detector* d);

/* Same ordering rule as ksm_set_stream: work already enqueued on the old stream is ordered in front of work on the new one
 * (an event is recorded on the OLD stream, so a stream handed in here must stay alive until the next kse_set_stream /
 * kse_destroy of this object). */
int kse_set_stream(kse_detector* d, void* hip_stream);
int kse_synchronize(kse_detector* d);

/* Detect in nrows rows from device memory: row i is the nbins floats at rows_dev + i * row_stride (in floats, >= nbins).
 * Asynchronous on the object's stream, no synchronisation inside.  rows_dev is 4-byte aligned and nothing more is required
 * (16-byte loads are used when base, stride and nbins allow them, otherwise 4-byte loads).  nrows = 0 is a successful no-op.
 * row_count_dev may be NULL; otherwise it receives int32[nrows], the emissions of every row.  floor_dev may be NULL;
 * otherwise it receives float32[nrows][nbins], contiguous: the pooled estimate (float)(SL+SR) / (float)(CL+CR) * 2^-6 of every
 * bin in every mode (a line to plot), NaN where CL+CR = 0. */
int kse_detect_rows_dev(kse_detector* d, const float* rows_dev, int64_t row_stride, int64_t nrows, int32_t* row_count_dev,
                        float* floor_dev);
/* Detect in nrows contiguous rows (host[nrows][nbins]); staged in pieces through library-owned device memory; synchronises. */
int kse_detect_rows(kse_detector* d, const float* rows_host, int64_t nrows);

/* Replace the detection parameters; the same checks as kse_create.  Rows already enqueued use the old values.  Hits,
 * rows_seen and emissions are kept. */
int kse_set_params(kse_detector* d, int32_t train, int32_t guard, float threshold_db, int32_t mode, int32_t min_width,
                   int32_t max_gap);
/* The index the next row gets (and rows_seen) becomes row_base >= 0. */
int kse_set_row_base(kse_detector* d, int64_t row_base);

/* Copy the hits to host int64[nbins] (hits_host may be NULL to fetch rows_seen alone) and return rows_seen (rows_seen may be
 * NULL); not both NULL.  Synchronises. */
int kse_read_hits(kse_detector* d, int64_t* hits_host, int64_t* rows_seen);
/* Copy the first min(stored, max_records) emission records to records_host (kse_emission[]; may be NULL to fetch the two
 * counts alone), *stored = records in the buffer = min(total, capacity), *total = emissions_total; either count pointer may be
 * NULL.  Synchronises. */
int kse_read_emissions(kse_detector* d, void* records_host, int64_t max_records, int64_t* stored, int64_t* total);
/* Device addresses, valid until kse_destroy: zero-copy for torch.  hits: int64[nbins].  emissions: kse_emission[capacity] and
 * the int64 emissions_total (either out pointer of kse_emissions_dev may be NULL, not both). */
int kse_hits_dev(kse_detector* d, int64_t** hits_dev);
int kse_emissions_dev(kse_detector* d, void** records_dev, int64_t** emissions_total_dev);

/* hits += hits_dev (int64[nbins] on the same device), rows_seen += rows_seen_add (>= 0): the multi-GPU sum of occupancy.
 * Emission lists are not merged: kse_set_row_base lets each rank number its rows globally and the caller concatenate.
 * Asynchronous. */
int kse_merge_hits_dev(kse_detector* d, const int64_t* hits_dev, int64_t rows_seen_add);
/* Empty the emission buffer and zero emissions_total; hits and rows_seen stay.  Asynchronous. */
int kse_clear_emissions(kse_detector* d);
/* Zero hits, rows_seen, the emission buffer and emissions_total.  Asynchronous. */
int kse_reset(kse_detector* d);

/* The detection kernel of the last kse_detect_rows_dev launch (before any: the form an aligned, contiguous buffer gets):
 * threads per workgroup, LDS bytes per workgroup, VGPRs, workgroups (before any launch: of one that fills the device),
 * vec = 1 for the 16-byte-load form and 0 for the 4-byte one, and the rows a workgroup holds side by side.  Any out pointer
 * may be NULL. */
int kse_kernel_info(kse_detector* d, int32_t* threads, int32_t* lds_bytes, int32_t* vgprs, int32_t* grid, int32_t* vec,
                    int32_t* rows_per_wg);

#ifdef __cplusplus
}
#endif

#endif
