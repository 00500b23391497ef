/* libksa_mask -- C ABI of the frequency-mask trigger and per-bin occupancy counter on the MI355X (gfx950): a companion of
 * libksa.
 *
 * A mask object compares every spectrum against an upper and a lower limit line.  It reports the frames that cross a line
 * (which, where and by how much) and counts, per bin, the spectra that crossed.  It consumes the per-frame dB rows that
 * libksa's entry points deliver in device memory (cur_db_dev of ksa_frames_dev, out_dev of ksa_curscan_dev with KSA_OUT_DB)
 * and nothing else of libksa: the libraries share no symbol, no state and no header.  The reference
 * (hanishkvc/prgs-sdr-kspecanal) has no counterpart.
 *
 * Conventions are those of ksa.h and ksa_density.h: plain C types only; 0 = success, non-zero = error with text in
 * ksm_last_error() (thread local).  "host" pointers are ordinary CPU memory, "dev" pointers are HIP device memory of the
 * object's device.  One object = one GPU; no concurrent calls on one object.  All device work is enqueued on the object's
 * stream (ksm_set_stream); entry points that take or fill host memory synchronise that stream before returning, the others
 * do not synchronise.  Every entry point selects its object's device for its own duration and hands the caller's current
 * HIP device back on return.  The library reads no environment variable.  A hipStream_t travels as void*.
 *
 * Semantics (the contract of every layer):
 *
 * A mask object is created with:
 * - nbins, 16 .. 1048576: the row length, i.e. the engine's fft_size.
 * - upper[nbins], host float32.
 * - lower[nbins], host float32; NULL means no lower line, i.e. all -inf.
 * - min_bins >= 1 (and <= nbins).
 * - an event capacity, 1 .. 2^20.
 * upper = +inf or lower = -inf disables that line at that bin; any infinity is allowed.  Refused, with their own text and a
 * null handle: a NaN in either line; lower[b] > upper[b]; nbins, min_bins or capacity out of range; min_bins > nbins.
 *
 * The object owns on the device int64 hits[3][nbins] (over, under, NaN; zero at creation), an event buffer of `capacity`
 * records and an int64 events_total.  The host object holds rows_seen, which is also the index the next row gets;
 * ksm_set_row_base overwrites it.
 *
 * Per-bin rule.  For every bin b of a row r, x = r[b] in float32:
 *
 *   nan   = x != x
 *   over  = x > upper[b]                     excess = x - upper[b]      one float32 subtraction, round to nearest
 *   under = x < lower[b]                     excess = lower[b] - x      (a bin cannot be both: lower <= upper)
 *   hits[0][b] += over;  hits[1][b] += under;  hits[2][b] += nan
 *
 * A NaN compares false, so it is neither over nor under.  With the infinities allowed above no excess is ever inf - inf.
 *
 * Per row:
 * - nover, nunder and nnan are the three counts over the bins.
 * - The peak is the over or under bin with the largest excess; among equal excesses (+inf included) the lowest bin wins.
 * - peak_kind is 0 for over, 1 for under, and -1 when nover + nunder == 0; then peak_bin = -1 and peak_excess = 0.
 * - The row is an event when nover + nunder >= min_bins or nnan > 0.
 *
 * An event record is the 32 bytes of ksm_event below.  Its `row` is the running index: rows_seen before the call plus the
 * row's position in the call.
 * - The buffer holds the FIRST `capacity` events since the last reset or clear, in ASCENDING row order, within a call and
 *   across calls.
 * - events_total counts every event, stored or not.
 * - Hits are counted for every row whether or not the buffer is full.
 * - The results never depend on grid, chunking or arrival order.  There are no float atomics anywhere (the peak is found
 *   with an integer maximum over a key that orders like the float).
 *
 * Refused per call, leaving everything as it was: null required pointers, nrows < 0, row_stride < nbins, max_records < 0,
 * a negative row base, a negative rows_seen_add.
 */
#ifndef KSA_MASK_H
#define KSA_MASK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KSM_ABI_VERSION 1 /* A binding takes the number from ksm_abi_version() of the library it loaded. */
#define KSM_MIN_NBINS 16
#define KSM_MAX_NBINS 1048576
#define KSM_MAX_CAPACITY 1048576
#define KSM_KIND_OVER 0
#define KSM_KIND_UNDER 1
#define KSM_KIND_NONE (-1)

typedef struct ksm_mask ksm_mask;

typedef struct ksm_event {
  int64_t row;       /* running row index */
  int32_t nover;     /* bins above the upper line */
  int32_t nunder;    /* bins below the lower line */
  int32_t nnan;      /* NaN bins */
  int32_t peak_bin;  /* -1 when nover + nunder == 0 */
  float peak_excess; /* 0 when nover + nunder == 0 */
  int32_t peak_kind; /* KSM_KIND_OVER, KSM_KIND_UNDER or KSM_KIND_NONE */
} ksm_event;

int ksm_abi_version(void);
const char* ksm_last_error(void);

/* A mask object on `device` with zeroed hits and no event, its stream the NULL stream.  *out is NULL when refused. */
int ksm_create(int32_t device, int32_t nbins, const float* upper_host, const float* lower_host, int32_t min_bins,
               int32_t capacity, ksm_mask** out);
void ksm_destroy(ksm_mask* m);

/* Same ordering rule as ksa_set_stream: work already enqueued on the old stream is ordered in front of work on the new one
 * (an event is recorded on the OLD stream, so a stream handed in here must stay alive until the next ksm_set_stream /
 * ksm_destroy of this object). */
int ksm_set_stream(ksm_mask* m, void* hip_stream);
int ksm_synchronize(ksm_mask* m);

/* Check nrows rows from device memory: row i is the nbins floats at rows_dev + i * row_stride (in floats, >= nbins).
 * Asynchronous on the object's stream, no synchronisation inside.  rows_dev is 4-byte aligned and nothing more is required
 * (16-byte loads are used when base and stride allow them).  nrows = 0 is a successful no-op.  row_event_dev may be NULL;
 * otherwise it receives [nrows] bytes, 1 where the row is an event and 0 elsewhere. */
int ksm_check_rows_dev(ksm_mask* m, const float* rows_dev, int64_t row_stride, int64_t nrows, uint8_t* row_event_dev);
/* Check nrows contiguous rows (host[nrows][nbins]); staged through library-owned device memory; synchronises. */
int ksm_check_rows(ksm_mask* m, const float* rows_host, int64_t nrows);

/* Replace the lines (lower_host may be NULL: no lower line); the same checks as ksm_create.  Rows already enqueued are
 * checked against the old lines.  Hits, rows_seen and events are kept.  Synchronises. */
int ksm_set_mask(ksm_mask* m, const float* upper_host, const float* lower_host);
/* The index the next row gets (and rows_seen) becomes row_base >= 0. */
int ksm_set_row_base(ksm_mask* m, int64_t row_base);

/* Copy the hits to host int64[3][nbins] (hits_host may be NULL to fetch rows_seen alone) and return rows_seen (rows_seen
 * may be NULL); not both NULL.  Synchronises. */
int ksm_read_hits(ksm_mask* m, int64_t* hits_host, int64_t* rows_seen);
/* Copy the first min(stored, max_records) event records to records_host (ksm_event[]; may be NULL to fetch the two counts
 * alone), *stored = records in the buffer = min(total, capacity), *total = events_total; either count pointer may be NULL.
 * Synchronises. */
int ksm_read_events(ksm_mask* m, void* records_host, int64_t max_records, int64_t* stored, int64_t* total);
/* Device addresses, valid until ksm_destroy: zero-copy for torch.  hits: int64[3][nbins].  events: ksm_event[capacity] and
 * the int64 events_total (either out pointer of ksm_events_dev may be NULL, not both). */
int ksm_hits_dev(ksm_mask* m, int64_t** hits_dev);
int ksm_events_dev(ksm_mask* m, void** records_dev, int64_t** events_total_dev);

/* hits += hits_dev (int64[3][nbins] on the same device), rows_seen += rows_seen_add (>= 0): the multi-GPU sum of occupancy.
 * Event lists are not merged: ksm_set_row_base lets each rank number its rows globally and the caller concatenate.
 * Asynchronous. */
int ksm_merge_hits_dev(ksm_mask* m, const int64_t* hits_dev, int64_t rows_seen_add);
/* Empty the event buffer and zero events_total; hits and rows_seen stay.  Asynchronous. */
int ksm_clear_events(ksm_mask* m);
/* Zero hits, rows_seen, the event buffer and events_total.  Asynchronous. */
int ksm_reset(ksm_mask* m);

/* The check kernel of the last ksm_check_rows_dev launch (before any: the form an aligned, contiguous buffer gets):
 * threads per workgroup, static LDS bytes, VGPRs, workgroups (before any launch: of one that fills the device),
 * vec = 1 for the 16-byte-load form and 0 for the 4-byte one.  Any out pointer may be NULL. */
int ksm_kernel_info(ksm_mask* m, int32_t* threads, int32_t* lds_bytes, int32_t* vgprs, int32_t* grid, int32_t* vec);

#ifdef __cplusplus
}
#endif

#endif
