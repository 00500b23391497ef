/* libksa_measure -- C ABI of the band measurements on the MI355X (gfx950): a companion of libksa.
 *
 * A meter object measures windows of dB rows: the integrated (channel) power, the power moments that give centroid and RMS
 * width, the peak, the occupied bandwidth (the width that holds a share beta of the power, the 99 % width for beta = 0.99)
 * and the x-dB width.  A window is either the span of an emission record, widened by a margin -- the records of libksa_detect
 * are read where they lie in device memory, with the count that lies beside them -- or one of a fixed list of bands
 * (channels), measured in every row.  The rows are the per-frame dB rows that libksa's entry points deliver in device memory
 * (cur_db_dev of ksa_frames_dev, out_dev of ksa_curscan_dev with KSA_OUT_DB).  The libraries share no symbol, no state and no
 * header: the layout of a span record is restated below.  The reference (hanishkvc/prgs-sdr-kspecanal) has no counterpart.
 *
 * Conventions are those of ksa_detect.h: plain C types only; 0 = success, non-zero = error with text in the last-error call
 * (thread local).  "host" pointers are ordinary CPU memory, "dev" pointers are HIP device memory of the object's device.  One
 * object = one GPU; no concurrent calls on one object.  All device work is enqueued on the object's stream; entry points that
 * take or fill host memory synchronise that stream before returning, the _dev ones do not synchronise.  Every entry point
 * selects its object's device for its own duration and hands the caller's current HIP device back on return.  The library
 * reads no environment variable.  Argument checks come before any HIP call.  A hipStream_t travels as void*.
 *
 * Semantics (the contract of every layer).
 *
 * A meter object is created with:
 * - device >= 0.
 * - nbins, 1 .. 2^24: the row length.
 * - capacity, 1 .. 2^20 result records, zero at creation.
 * - occupied, float32, 0.5 <= beta < 1: the share of the power inside the occupied bandwidth.
 * - xdb, float32, finite, 0 .. 100: how far below the peak the x-dB edges lie.
 * - margin, 0 .. 65536 bins: how far a span is widened on either side before it is measured.
 * Each out-of-range parameter is refused with its own text and a null handle.  The set-params call replaces the last three;
 * a launch carries its parameters by value, so work already enqueued keeps the old ones.
 *
 * A task is a row r and an inclusive window [a, b] with 0 <= a <= b < nbins.  For bin k, x = r[k] in float32:
 *
 *   valid = !(x != x) && x != -inf
 *   xc    = fminf(fmaxf(x, -500), 500)                  the detector's rule: +inf counts as 500
 *   p_k   = 10^((double)xc / 10)                        in float64; an invalid bin has p_k = 0 and is never the peak
 *
 * The result is the 80 bytes of kme_result below:
 * - row: the running index of the row; bin_lo, bin_hi = a, b: the window that was summed; nvalid: its valid bins.
 * - power = sum of p_k; power_db = (float) (10 * log10(power)), -inf when nvalid = 0.
 * - m1 = sum of p_k * (k - a), m2 = sum of p_k * (k - a)^2: centroid = a + m1 / power, variance = m2 / power - (m1 / power)^2.
 * - peak_bin: the valid bin with the largest xc, the lowest bin among equals (+0 and -0 are equal); peak_db: the row's own
 *   float32 at that bin, bit for bit.  -1 and NaN when nvalid = 0.
 * - obw_lo, obw_hi.  With tail = (1 - (double)beta) / 2 * power: obw_lo is the smallest k whose sum of p over [a, k] exceeds
 *   tail, obw_hi the largest k whose sum of p over [k, b] exceeds tail.  Both -1 when nvalid = 0.
 * - xdb_lo, xdb_hi: the lowest and the highest valid bin of the window with xc >= xc[peak_bin] - xdb, the subtraction and the
 *   comparison in float32.  Both -1 when nvalid = 0.
 * - flags: KME_FLAG_MEASURED, KME_FLAG_CLIPPED (a row edge cut the widened window), KME_FLAG_INVALID (nvalid < b - a + 1).
 *
 * Sums are float64 and ANY summation order is allowed: the relative error of power, m1 and m2 is at most (b - a + 1) * 2^-53
 * (every term is >= 0), plus the error of the float64 10^x.  An OBW edge is therefore exact wherever no partial sum next to it
 * comes within that distance of tail; every integer field and peak_db are exact otherwise.  There are no float atomics
 * anywhere: a result is written once, by the one wave or workgroup that measured it.
 *
 * Refused per call, leaving everything as it was: null required pointers, negative counts, row_stride < nbins, a rows
 * pointer that is not 4-byte aligned, a span stride below 16 or no multiple of 8, first < 0, a negative row base, result
 * slots beyond capacity.
 */
#ifndef KSA_MEASURE_H
#define KSA_MEASURE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KME_ABI_VERSION 1 /* A binding takes the number from the library it loaded. */
#define KME_MAX_NBINS 16777216
#define KME_MAX_CAPACITY 1048576
#define KME_MAX_MARGIN 65536
#define KME_MAX_BANDS 1024
#define KME_WAVE_MAX_BINS 256 /* windows up to this width go to the wave form, wider ones to the workgroup form */
#define KME_FLAG_MEASURED 1
#define KME_FLAG_CLIPPED 2
#define KME_FLAG_INVALID 4

typedef struct kme_meter kme_meter;

/* What a span record begins with; records lie span_stride_bytes apart (>= 16, a multiple of 8) and may be longer: the 32
 * bytes of libksa_detect's emission record begin like this. */
typedef struct kme_span {
  int64_t row;    /* running row index */
  int32_t bin_lo; /* first bin */
  int32_t bin_hi; /* last bin, inclusive */
} kme_span;

typedef struct kme_result {
  int64_t row;      /* running row index */
  int32_t bin_lo;   /* first bin of the window that was summed */
  int32_t bin_hi;   /* its last bin, inclusive */
  int32_t nvalid;   /* valid bins in the window */
  int32_t flags;    /* KME_FLAG_*; 0 = the slot was never written */
  double power;     /* sum of p_k */
  double m1;        /* sum of p_k * (k - bin_lo) */
  double m2;        /* sum of p_k * (k - bin_lo)^2 */
  int32_t peak_bin; /* the valid bin with the largest xc, the lowest among equals; -1 without a valid bin */
  float peak_db;    /* the row's float32 at peak_bin; NaN without a valid bin */
  int32_t obw_lo;   /* occupied bandwidth, first bin */
  int32_t obw_hi;   /* occupied bandwidth, last bin */
  int32_t xdb_lo;   /* x-dB width, first bin */
  int32_t xdb_hi;   /* x-dB width, last bin */
  float power_db;   /* 10 log10(power); -inf without a valid bin */
  int32_t reserved; /* 0 */
} kme_result;

int kme_abi_version(void);
const char* kme_last_error(void);

/* A meter object on `device` with zeroed results and no band, its stream the NULL stream.  *out is NULL when refused. */
int kme_create(int32_t device, int32_t nbins, int32_t capacity, float occupied, float xdb, int32_t margin, kme_meter** out);
void kme_destroy(kme_meter* m);

/* Work already enqueued on the old stream is ordered in front of work on the new one (an event is recorded on the OLD
 * stream, so a stream handed in here must stay alive until it is replaced or the object destroyed). */
int kme_set_stream(kme_meter* m, void* hip_stream);
int kme_synchronize(kme_meter* m);

/* Replace occupied, xdb and margin; the same checks as at creation.  Results are kept. */
int kme_set_params(kme_meter* m, float occupied, float xdb, int32_t margin);

/* Measure spans.  Row i of the batch is the nbins floats at rows_dev + i * row_stride (in floats, >= nbins) and has the
 * running index row_base + i; rows_dev is 4-byte aligned and nothing more is required (16-byte loads are used when base,
 * stride and nbins allow them, otherwise 4-byte loads).  Span i is the kme_span at spans_dev + i * span_stride_bytes;
 * *total_dev (int64, device memory) counts the spans and is read on the device, so the host never waits for whoever
 * writes the list.  For every i in [first, min(*total_dev, span_capacity, capacity)) whose row lies in
 * [row_base, row_base + nrows), results[i] becomes the measurement of [bin_lo - margin, bin_hi + margin], clipped to the row,
 * in row `row - row_base` of the batch.  Every other slot is left as it was; so is the slot of a span with bin_lo < 0,
 * bin_hi >= nbins or bin_lo > bin_hi.  The slot is the span's own index: result i pairs with span i whatever order the
 * work runs in.  Asynchronous. */
int kme_measure_spans_dev(kme_meter* m, const float* rows_dev, int64_t row_stride, int64_t nrows, int64_t row_base,
                          const void* spans_dev, int64_t span_stride_bytes, const int64_t* total_dev, int64_t span_capacity,
                          int64_t first);
/* The same over nrows contiguous rows in host memory (host[nrows][nbins]), staged in pieces through library-owned device
 * memory; the spans and their count stay on the device.  Synchronises. */
int kme_measure_spans(kme_meter* m, const float* rows_host, int64_t nrows, int64_t row_base, const void* spans_dev,
                      int64_t span_stride_bytes, const int64_t* total_dev, int64_t span_capacity, int64_t first);

/* The fixed bands: bands_host is int32[nb][2], lo and hi (inclusive) of every band, 0 <= lo <= hi < nbins, nb 0 .. 1024
 * (bands_host may be NULL when nb = 0).  They hold for the launches that follow.  Synchronises. */
int kme_set_bands(kme_meter* m, const int32_t* bands_host, int32_t nb);
/* Measure every band in every row: results[first_slot + r * nb + j] becomes the measurement of band j (no margin) in row r
 * of the batch, its row field row_base + r.  Refused when first_slot < 0 or first_slot + nrows * nb > capacity.
 * Asynchronous. */
int kme_measure_bands_dev(kme_meter* m, const float* rows_dev, int64_t row_stride, int64_t nrows, int64_t row_base,
                          int64_t first_slot);
/* The same over contiguous rows in host memory.  Synchronises. */
int kme_measure_bands(kme_meter* m, const float* rows_host, int64_t nrows, int64_t row_base, int64_t first_slot);

/* Copy results[first .. first + count) to out_host (kme_result[count]); first >= 0, count >= 0, first + count <= capacity.
 * Synchronises. */
int kme_read_results(kme_meter* m, void* out_host, int64_t first, int64_t count);
/* The device address of kme_result[capacity], valid until the object is destroyed: zero-copy for torch. */
int kme_results_dev(kme_meter* m, void** results_dev);
/* Zero every result slot.  Asynchronous. */
int kme_reset(kme_meter* m);

/* The kernel launched last (before any launch: the wave form with 16-byte loads if nbins allows them): threads per
 * workgroup, static LDS bytes, VGPRs, workgroups, vec = 1 for the 16-byte-load form and 0 for the 4-byte one, form = 0 for
 * the wave form (one 64-lane wave per task, four tasks per workgroup) and 1 for the workgroup form (one workgroup per task).
 * A spans call launches both forms, the workgroup form last; a bands call launches the forms its band widths need.  Any
 * out pointer may be NULL. */
int kme_kernel_info(kme_meter* m, int32_t* threads, int32_t* lds_bytes, int32_t* vgprs, int32_t* grid, int32_t* vec,
                    int32_t* form);

#ifdef __cplusplus
}
#endif

#endif
