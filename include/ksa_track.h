/* libksa_track -- C ABI of the emission linker and track list on the MI355X (gfx950): a companion of libksa.
 *
 * A tracker joins the per-row emissions of a CFAR detector (row, bin_lo, bin_hi, peak, floor: "where in frequency, one
 * spectrum at a time") into time-frequency tracks: a carrier of 400 rows, a burst of 10, a chirp of 60 one-bin steps become one
 * record each, with its first and last row, its occupied band, its peak and what its drift is read from (a signal list).  The
 * linking is a connected-component labelling over a sorted interval list: a union-find across rows, per-component reductions
 * and an ordered compaction, all in integers.  The input record has the byte layout of libksa_detect's kse_emission, so that
 * detector's device buffer is linked where it lies; the two libraries still share no symbol, no state and no header, and this
 * one shares none with libksa or the other companions.  The reference (hanishkvc/prgs-sdr-kspecanal) has no counterpart.
 *
 * Conventions are those of the other headers: plain C types only; 0 = success, non-zero = error with text in
 * ktr_last_error() (thread local).  "host" pointers are ordinary CPU memory, "dev" pointers are HIP device memory of the
 * object's device.  One object = one GPU; no concurrent calls on one object.  All device work is enqueued on the object's
 * stream (ktr_set_stream); entry points that take or fill host memory synchronise that stream before returning, the `_dev`
 * ones do not synchronise.  Every entry point selects its object's device for its own duration and hands the caller's current
 * HIP device back on return.  The library reads no environment variable.  Argument checks come before any HIP call.  A
 * hipStream_t travels as void*.
 *
 * Semantics (the contract of every layer).  Every decision is an integer, so the results never depend on grid, tile or arrival
 * order.
 *
 * Input: n spans, each the 32 bytes of ktr_span below, in strictly ascending (row, bin_lo) order.  Index i is VALID iff
 *   0 <= bin_lo[i] <= bin_hi[i] < nbins,   0 <= row[i] < row_end,
 *   and for i > 0: row[i] > row[i-1], or row[i] == row[i-1] and bin_lo[i] > bin_lo[i-1] and bin_lo[i] > bin_hi[i-1].
 * peak_bin, ndet, peak_db and floor_db are carried, never judged.
 *
 * The object is created with:
 * - device >= 0.
 * - nbins, 1 .. 2^24: the row length.
 * - max_spans, 1 .. 2^22: the largest n of a link (the work memory is about 72 bytes per span).
 * - row_gap, 0 .. 1024: rows that may be missing between two linked spans.
 * - bin_slop, 0 .. nbins: bins by which two spans may miss each other and still be linked.
 * - min_rows >= 1, min_spans >= 1: the filter below.
 * - capacity, 1 .. 2^20 track records.
 * Each out-of-range parameter is refused with its own text and a null handle.  ktr_set_params replaces row_gap, bin_slop,
 * min_rows and min_spans with the same checks.
 *
 * Adjacency.  Spans i < j are adjacent iff, compared in int64,
 *   1 <= row[j] - row[i] <= 1 + row_gap   and   bin_lo[i] <= bin_hi[j] + bin_slop   and   bin_lo[j] <= bin_hi[i] + bin_slop.
 * Spans of one row are never adjacent.  A component is a connected component of that graph; its id is the lowest span index
 * in it, first_span.
 *
 * Record: the 80 bytes of ktr_track below.  The peak span of a component is the member with the largest key(peak_db), the
 * lowest index among equals, where for u = the float32's bits key = ~u if the sign bit of u is set and u | 0x80000000
 * otherwise: a total order on bit patterns (-inf < -1 < -0 < +0 < 1 < +inf < the positive NaNs), so NaN needs no special case.
 * flags bit 0, KTR_FLAG_OPEN_END, is set when row_last + row_gap + 1 >= row_end: a span of a row that has not arrived yet
 * could still join the track.
 *
 * Filter and order.  A component is a track iff row_last - row_first + 1 >= min_rows and nspans >= min_spans.
 * - components_total counts every component, tracks_total every track.
 * - The buffer holds the FIRST `capacity` tracks in ascending first_span order, which is ascending (row_first, bin_lo of the
 *   first span) order.
 * - labels[i] is the rank of span i's track in that order (it may be >= capacity), -1 when its component was filtered out.
 * - There are no float atomics anywhere: peak_db and floor_db are copied from the peak span, bit for bit.
 *
 * Bad input.  bad_spans is the number of indices that are not valid.  When it is non-zero nothing is linked: both totals are
 * 0, every label is -1 and no kernel walks the list.  ktr_link (host memory) refuses such a list before any HIP call and names
 * the first offending index; ktr_link_dev (device memory) cannot, and reports the count through ktr_read_tracks.
 *
 * Each link REPLACES the previous result.  Relinking a longer prefix of the same list is the supported way to follow a running
 * capture, and it is idempotent.  n = 0 is a successful link with empty results.
 *
 * Refused per call, leaving the state as it was: a null object or required pointer, n < 0, n > max_spans, row_end < 0,
 * max_records < 0, max_labels < 0.
 *
 * Out of scope: an incremental stream form that carries open tracks across calls (KTR_FLAG_OPEN_END says which tracks a
 * relink could extend), and merging the track lists of several GPUs: each rank's detector already numbers its rows globally
 * (kse_set_row_base), so the caller concatenates the emissions and links once.
 */
#ifndef KSA_TRACK_H
#define KSA_TRACK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KTR_ABI_VERSION 1 /* A binding takes the number from ktr_abi_version() of the library it loaded. */
#define KTR_MAX_NBINS 16777216 /* 2^24 */
#define KTR_MAX_SPANS 4194304 /* 2^22 */
#define KTR_MAX_ROW_GAP 1024
#define KTR_MAX_CAPACITY 1048576 /* 2^20 */
#define KTR_FLAG_OPEN_END 1 /* row_last + row_gap + 1 >= row_end */

typedef struct ktr_tracker ktr_tracker;

/* One span: byte for byte the kse_emission of ksa_detect.h. */
typedef struct ktr_span {
  int64_t row;      /* running row index */
  int32_t bin_lo;   /* first bin */
  int32_t bin_hi;   /* last bin (inclusive) */
  int32_t peak_bin; /* carried into the track of which this is the peak span */
  int32_t ndet;     /* not read */
  float peak_db;    /* orders the peak spans, by its bits */
  float floor_db;   /* carried with peak_db */
} ktr_span;

/* One track.  The struct has no padding: 80 bytes in all. */
typedef struct ktr_track {
  int64_t row_first;  /* first row of the component */
  int64_t row_last;   /* last row of the component */
  int64_t peak_row;   /* row of the peak span */
  int64_t cells;      /* the sum of bin_hi - bin_lo + 1 over the members */
  int64_t sum_mid2;   /* the sum of bin_lo + bin_hi over the members: twice the sum of their centres */
  int32_t bin_lo;     /* the lowest bin_lo of the members */
  int32_t bin_hi;     /* the highest bin_hi of the members */
  int32_t nspans;     /* member spans */
  int32_t peak_bin;   /* peak_bin of the peak span */
  int32_t mid2_first; /* bin_lo + bin_hi of the member with the lowest index */
  int32_t mid2_last;  /* bin_lo + bin_hi of the member with the highest index */
  int32_t first_span; /* the component id: the lowest index of the members */
  int32_t flags;      /* bit 0: KTR_FLAG_OPEN_END */
  float peak_db;      /* of the peak span, bit for bit */
  float floor_db;     /* of the peak span, bit for bit */
} ktr_track;

int ktr_abi_version(void);
const char* ktr_last_error(void);

/* A tracker on `device` with no result, its stream the NULL stream.  *out is NULL when refused. */
int ktr_create(int32_t device, int32_t nbins, int32_t max_spans, int32_t row_gap, int32_t bin_slop, int32_t min_rows,
               int32_t min_spans, int32_t capacity, ktr_tracker** out);
void ktr_destroy(ktr_tracker* t);

/* Work already enqueued on the old stream is ordered in front of work on the new one (an event is recorded on the OLD stream,
 * so a stream handed in here must stay alive until the next ktr_set_stream / ktr_destroy of this object). */
int ktr_set_stream(ktr_tracker* t, void* hip_stream);
int ktr_synchronize(ktr_tracker* t);

/* Replace row_gap, bin_slop, min_rows and min_spans (the same checks as ktr_create); links already enqueued use the old
 * values. */
int ktr_set_params(ktr_tracker* t, int32_t row_gap, int32_t bin_slop, int32_t min_rows, int32_t min_spans);

/* Link spans in device memory (ktr_span[n_max], 8-byte aligned; n_max <= max_spans).  n_dev may be NULL: n = n_max.
 * Otherwise it is one int64 in device memory and n = min(max(*n_dev, 0), n_max) is read ON THE DEVICE, so a detector's
 * buffer and its emissions_total (kse_emissions_dev) flow in without a host round trip.  labels_dev may be NULL; otherwise it
 * receives int32 [n_max], -1 from index n on.  Asynchronous, no synchronisation inside. */
int ktr_link_dev(ktr_tracker* t, const void* spans_dev, int64_t n_max, const int64_t* n_dev, int64_t row_end,
                 int32_t* labels_dev);
/* The same from host memory (ktr_span[n]; labels_host int32 [n] or NULL); a list with an index that is not valid is refused
 * before any HIP call.  Staged through library-owned device memory; synchronises. */
int ktr_link(ktr_tracker* t, const void* spans_host, int64_t n, int64_t row_end, int32_t* labels_host);

/* Copy the first min(stored, max_records) track records to records_host (ktr_track[]; may be NULL to fetch the counts alone),
 * *stored = records in the buffer = min(tracks_total, capacity), *total = tracks_total, *components = components_total,
 * *bad_spans as defined above; any count pointer may be NULL.  Synchronises. */
int ktr_read_tracks(ktr_tracker* t, void* records_host, int64_t max_records, int64_t* stored, int64_t* total,
                    int64_t* components, int64_t* bad_spans);
/* Copy the first min(n, max_labels) labels of the last link to labels_host (int32 []; may be NULL) and return its n in
 * *n_spans (may be NULL); not both NULL.  Synchronises. */
int ktr_read_labels(ktr_tracker* t, int32_t* labels_host, int64_t max_labels, int64_t* n_spans);
/* Device addresses, valid until ktr_destroy: ktr_track[capacity] and int64 [4] = tracks_total, components_total, bad_spans,
 * n of the last link (either out pointer may be NULL, not both). */
int ktr_tracks_dev(ktr_tracker* t, void** records_dev, int64_t** counters_dev);
/* No result: the four counters zero.  Asynchronous. */
int ktr_clear(ktr_tracker* t);

/* The link kernel: threads per workgroup, LDS bytes per workgroup, VGPRs, the workgroups of its last launch (before any: of
 * max_spans spans) and the number of launches a link takes.  Any out pointer may be NULL. */
int ktr_kernel_info(ktr_tracker* t, int32_t* threads, int32_t* lds_bytes, int32_t* vgprs, int32_t* grid, int32_t* launches);

#ifdef __cplusplus
}
#endif

#endif
