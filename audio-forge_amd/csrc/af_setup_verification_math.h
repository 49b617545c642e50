/* af_setup_verification_math.h -- the measurements of validate_voice_setup_verification (python/mic_eq/analysis/voice_setup.py
 * :1446-1679) in f64 on plain arrays: the adaptive house curve (auto_eq_parts/target.py:8-104 over TARGET_CURVES and
 * EQ_FREQUENCIES of config_parts), _shape_error_db (:1446-1465), the repeatability delta (:1562-1575), the four band medians of
 * the spectral SNR (:1634-1645) and the levels (_rms_db :102-106, the clipped tests :1490 and :1677).  Plain C, shared by
 * af_api_setup_verification.cpp, tests/ref/setup_verification_ref.c and, for the per-element rules marked SVM_FN, the kernels of
 * af_setup_verification.hip (which define SVM_FN as a host-and-device qualifier before they include this file).
 *
 * ORDER OF THE SUMS.  Every sum over bins is an "svm sum": 256 lanes, lane t adds the terms t, t + 256, ... in that order
 * (a term outside its mask is +0.0), then p[t] += p[t + s] for s = 128, 64, ..., 1.  The kernels run exactly this, so their sums
 * are the restatement's bit for bit; NumPy adds pairwise in another order, which moves a result by rounding only.
 * The sum of squares of a signal is NumPy's own order, so that one is NumPy's bit for bit: the reduction walks the array in
 * buffers of 8192 terms and adds each buffer's sum to a running total that starts at 0; a buffer's sum is pairwise_sum of
 * loops_utils.h (blocks of at most 128 terms with eight running sums, halves cut at multiples of eight). */
#ifndef AF_SETUP_VERIFICATION_MATH_H
#define AF_SETUP_VERIFICATION_MATH_H
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/audioforge_mi.h"
#include "af_numpy_rules.h"

#ifndef SVM_FN
#define SVM_FN static inline
#endif

#define SVM_LANES 256
#define SVM_MASK_LOW 80.0       /* :1454, :1567-1569, both ends inclusive */
#define SVM_MASK_HIGH 12000.0
#define SVM_MIN_BINS 8          /* :1455 */
#define SVM_BANDS 10
#define SVM_PAIRWISE_BLOCK 128  /* PW_BLOCKSIZE */
#define SVM_PAIRWISE_BUFFER 8192 /* NPY_BUFSIZE: what one call of the reduction's inner loop sees */
#define SVM_PAIRWISE_DEPTH 8    /* halvings from a buffer down to a block, with room */

/* EQ_FREQUENCIES, config_parts/settings.py:11-22, and TARGET_CURVES' band_targets, config_parts/catalogs.py:105-126, in the
 * order of the AF_TARGET_* ids */
#define SVM_EQ_FREQUENCIES {80.0, 160.0, 320.0, 640.0, 1280.0, 2500.0, 5000.0, 8000.0, 12000.0, 16000.0}
#define SVM_TARGET_CURVES                                      \
  {{-2.0, -1.0, 0.0, 1.0, 2.0, 3.0, 2.0, 1.0, 0.0, -1.0},      \
   {0.0, 0.0, 1.0, 2.0, 3.0, 4.0, 3.0, 2.0, 1.0, 0.0},         \
   {-1.0, 0.0, 1.0, 2.0, 4.0, 5.0, 4.0, 2.0, 0.0, -2.0},       \
   {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}}
static const char *const svm_preset_names[AF_TARGET_PRESET_COUNT] = {"broadcast", "podcast", "streaming", "flat"};

SVM_FN double svm_clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); } /* np.clip; NaN stays */

/* np.interp(f, EQ_FREQUENCIES, band_targets, left=first, right=last), target.py:88-94 */
SVM_FN double svm_catalog_curve(int preset, double f) {
  const double xp[SVM_BANDS] = SVM_EQ_FREQUENCIES, curves[AF_TARGET_PRESET_COUNT][SVM_BANDS] = SVM_TARGET_CURVES;
  const double *fp = curves[preset];
  int lo = 0, hi = SVM_BANDS - 1;
  if (f < xp[0]) return fp[0];
  if (f >= xp[SVM_BANDS - 1]) return fp[SVM_BANDS - 1];
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (f >= xp[mid]) lo = mid; else hi = mid;
  }
  return (fp[lo + 1] - fp[lo]) / (xp[lo + 1] - xp[lo]) * (f - xp[lo]) + fp[lo];
}

/* what _adaptive_voice_offsets takes from the measured spectrum before it looks at a frequency, target.py:24-56 */
typedef struct svm_offset_scalars {
  double body_db, presence_db, sibilance_db, tilt_db_per_octave, low_mid_balance; /* reported (af_setup_verification_row) */
  double flat_scale;                                                              /* clip(-0.60 tilt_norm, -0.8, 0.8), :48 */
  double warmth_offset, presence_offset, sibilance_offset;                        /* :54-56 */
} svm_offset_scalars;

/* target.py:27-28 and :40-56 from the three band means and the regression's slope in dB per decade */
SVM_FN void svm_offset_rules(double body_db, double presence_db, double sibilance_db, double tilt_db_per_decade, svm_offset_scalars *o) {
  const double sibilance_ratio = svm_clip((sibilance_db - presence_db) / 7.0, -1.0, 1.0);
  double tilt_norm;
  o->body_db = body_db;
  o->presence_db = presence_db;
  o->sibilance_db = sibilance_db;
  o->low_mid_balance = svm_clip((body_db - presence_db) / 8.0, -1.0, 1.0);
  o->tilt_db_per_octave = tilt_db_per_decade * log10(2.0);
  tilt_norm = svm_clip(o->tilt_db_per_octave / 4.0, -1.0, 1.0);
  o->flat_scale = svm_clip(-0.60 * tilt_norm, -0.8, 0.8);
  o->warmth_offset = svm_clip(-0.9 * o->low_mid_balance, -1.2, 1.2);
  o->presence_offset = svm_clip(0.8 * o->low_mid_balance - 0.5 * tilt_norm, -1.5, 1.5);
  o->sibilance_offset = svm_clip(-1.2 * sibilance_ratio, -1.8, 1.2);
}

/* the abscissa of the tilt regression, target.py:30 */
SVM_FN double svm_log10_frequency(double f) { return log10(f < 20.0 ? 20.0 : f); }

SVM_FN double svm_gaussian(double safe, double centre, double width) { /* target.py:59-61 */
  const double l = log2(safe / centre);
  return exp(-(l * l) / (2.0 * (width * width)));
}

/* the offset at one frequency, target.py:45-62 */
SVM_FN double svm_offset_at(int preset, const svm_offset_scalars *o, double f) {
  double offset = 0.0;
  if (preset == AF_TARGET_FLAT) {
    const double xp[3] = {100.0, 1000.0, 8000.0}, fp[3] = {-1.0, 0.0, 1.0};
    double ramp;
    if (f < xp[0]) ramp = fp[0];
    else if (f >= xp[2]) ramp = fp[2];
    else {
      const int lo = f >= xp[1] ? 1 : 0;
      ramp = (fp[lo + 1] - fp[lo]) / (xp[lo + 1] - xp[lo]) * (f - xp[lo]) + fp[lo];
    }
    offset += o->flat_scale * ramp;
    return svm_clip(offset, -1.0, 1.0);
  }
  {
    const double safe = f < 20.0 ? 20.0 : f;
    offset += o->warmth_offset * svm_gaussian(safe, 350.0, 0.8);
    offset += o->presence_offset * svm_gaussian(safe, 2200.0, 0.9);
    offset += o->sibilance_offset * svm_gaussian(safe, 7000.0, 0.65);
  }
  return svm_clip(offset, -2.0, 2.0);
}

/* the first and the count of the bins of an ascending grid inside [low, high] (high_inclusive) or [low, high) */
SVM_FN void svm_bin_range(const double *freqs, int K, double low, double high, int high_inclusive, int *first, int *count) {
  int k, a = K, n = 0;
  for (k = 0; k < K; ++k)
    if (freqs[k] >= low && (high_inclusive ? freqs[k] <= high : freqs[k] < high)) {
      if (k < a) a = k;
      ++n;
    }
  *first = n ? a : 0;
  *count = n;
}

/* NumPy's pairwise sum of the squares of float32 samples taken to f64 first (audio = asarray(audio, float); audio * audio), one
 * block of at most SVM_PAIRWISE_BLOCK terms */
SVM_FN double svm_square(float x) { const double d = (double)x; return d * d; }
SVM_FN double svm_pairwise_block(const float *a, int64_t n) {
  double r[8], res;
  int64_t i;
  int j;
  if (n < 8) {
    res = 0.0;
    for (i = 0; i < n; ++i) res += svm_square(a[i]);
    return res;
  }
  for (j = 0; j < 8; ++j) r[j] = svm_square(a[j]);
  for (i = 8; i < n - (n % 8); i += 8)
    for (j = 0; j < 8; ++j) r[j] += svm_square(a[i + j]);
  res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += svm_square(a[i]);
  return res;
}

/* the left half of a node of more than SVM_PAIRWISE_BLOCK terms */
SVM_FN int64_t svm_pairwise_left(int64_t n) {
  int64_t half = n / 2;
  half -= half % 8;
  return half;
}

/* the whole recursion under one node of at most SVM_PAIRWISE_BUFFER terms, blocks from left to right: a finished right child is
 * added to its waiting left sibling */
SVM_FN double svm_pairwise_sum_squares(const float *a, int64_t n) {
  double waiting[SVM_PAIRWISE_DEPTH];
  int64_t lo = 0, len = n, right_len[SVM_PAIRWISE_DEPTH];
  uint64_t went_right = 0; /* bit d: the path took the right child below depth d */
  int depth = 0;
  double value;
  for (;;) {
    while (len > SVM_PAIRWISE_BLOCK) { /* down the left edge */
      const int64_t half = svm_pairwise_left(len);
      right_len[depth] = len - half;
      went_right &= ~((uint64_t)1 << depth);
      len = half;
      ++depth;
    }
    value = svm_pairwise_block(a + lo, len);
    lo += len;
    while (depth > 0 && ((went_right >> (depth - 1)) & 1)) { /* up while this was a right child */
      --depth;
      value = waiting[depth] + value;
    }
    if (depth == 0) return value;
    waiting[depth - 1] = value; /* a left child: its sibling comes next */
    went_right |= (uint64_t)1 << (depth - 1);
    len = right_len[depth - 1];
  }
}

/* np.sum(audio * audio) over a whole signal */
SVM_FN double svm_sum_squares(const float *a, int64_t n) {
  double total = 0.0;
  int64_t at;
  for (at = 0; at < n; at += SVM_PAIRWISE_BUFFER)
    total += svm_pairwise_sum_squares(a + at, n - at < SVM_PAIRWISE_BUFFER ? n - at : SVM_PAIRWISE_BUFFER);
  return total;
}

/* _rms_db, :102-106, from the sum of squares */
SVM_FN double svm_rms_db(double sum_squares, int64_t n) {
  if (n <= 0) return -120.0;
  return 20.0 * log10(sqrt(sum_squares / (double)n) + 1e-9);
}

/* ---- host only below: the reductions in the order stated at the top, and the sorts ------------------------------------- */
/* the svm sum of term(i), i < n; masked-out terms are +0.0 */
static inline double svm_sum_lanes(double *p /* [SVM_LANES], the lanes' running sums */) {
  int s, t;
  for (s = SVM_LANES / 2; s >= 1; s /= 2)
    for (t = 0; t < s; ++t) p[t] += p[t + s];
  return p[0];
}
static inline double svm_sum(const double *v, int n) {
  double p[SVM_LANES];
  int i;
  for (i = 0; i < SVM_LANES; ++i) p[i] = 0.0;
  for (i = 0; i < n; ++i) p[i % SVM_LANES] += v[i];
  return svm_sum_lanes(p);
}

static inline int svm_compare(const void *a, const void *b) { /* NaN last, as np.sort */
  const double x = *(const double *)a, y = *(const double *)b;
  if (x != x) return y != y ? 0 : 1;
  if (y != y) return -1;
  return (x > y) - (x < y);
}
/* np.median: NaN when any value is; `scratch` [n] is overwritten */
static inline double svm_median(const double *v, int n, double *scratch) {
  memcpy(scratch, v, sizeof(double) * (size_t)n);
  qsort(scratch, (size_t)n, sizeof(double), svm_compare);
  if (scratch[n - 1] != scratch[n - 1]) return scratch[n - 1];
  return af_median_sorted(scratch, n);
}

/* _band_mean, target.py:8-12, over n bins */
static inline double svm_band_mean(const double *freqs, const double *db, int n, double low, double high, double *work /* [n] */) {
  int i, count = 0;
  for (i = 0; i < n; ++i) {
    const int in = freqs[i] >= low && freqs[i] <= high;
    work[i] = in ? db[i] : 0.0;
    count += in;
  }
  if (!count) return svm_sum(db, n) / (double)n;
  return svm_sum(work, n) / (double)count;
}

/* target.py:24-43: the band means and the regression over 100-8000 Hz; n >= 1 */
static inline void svm_offset_scalars_of(const double *freqs, const double *db, int n, svm_offset_scalars *o, double *work /* [2 n] */) {
  const double body = svm_band_mean(freqs, db, n, 180.0, 800.0, work), presence = svm_band_mean(freqs, db, n, 1200.0, 3500.0, work);
  const double sibilance = svm_band_mean(freqs, db, n, 5500.0, 8500.0, work);
  double tilt = 0.0, *x = work, *y = work + n;
  int i, count = 0;
  for (i = 0; i < n; ++i) count += freqs[i] >= 100.0 && freqs[i] <= 8000.0;
  if (count >= 2) {
    double mean_x, mean_y, denom, dot;
    for (i = 0; i < n; ++i) {
      const int in = freqs[i] >= 100.0 && freqs[i] <= 8000.0;
      x[i] = in ? svm_log10_frequency(freqs[i]) : 0.0;
      y[i] = in ? db[i] : 0.0;
    }
    mean_x = svm_sum(x, n) / (double)count;
    mean_y = svm_sum(y, n) / (double)count;
    for (i = 0; i < n; ++i) {
      const int in = freqs[i] >= 100.0 && freqs[i] <= 8000.0;
      const double xc = x[i] - mean_x;
      y[i] = in ? xc * (y[i] - mean_y) : 0.0;
      x[i] = in ? xc * xc : 0.0;
    }
    denom = svm_sum(x, n);
    dot = svm_sum(y, n);
    if (denom > 0.0) tilt = dot / denom;
  }
  svm_offset_rules(body, presence, sibilance, tilt, o);
}

/* get_target_curve(freqs, preset, measured, "adaptive"), target.py:65-104, over n bins; measured_db null = the catalog curve */
static inline void svm_target_curve(const double *freqs, const double *measured_db, int n, int preset, double *target /* [n] */,
                                    svm_offset_scalars *scalars /* nullable */, double *work /* [2 n] */) {
  svm_offset_scalars o;
  int i;
  memset(&o, 0, sizeof o);
  for (i = 0; i < n; ++i) target[i] = svm_catalog_curve(preset, freqs[i]);
  if (measured_db && n > 0) {
    svm_offset_scalars_of(freqs, measured_db, n, &o, work);
    for (i = 0; i < n; ++i) target[i] = target[i] + svm_offset_at(preset, &o, freqs[i]);
  }
  if (scalars) *scalars = o;
}

/* the RMS of d[i] - median(d), i < n: :1463-1465 with d = measured - target once both medians are out, and :1574-1575 */
static inline double svm_centred_rms(const double *measured, const double *target, int n, double *work /* [2 n] */) {
  const double m0 = svm_median(measured, n, work), t0 = svm_median(target, n, work);
  int i;
  for (i = 0; i < n; ++i) {
    const double d = (measured[i] - m0) - (target[i] - t0);
    work[i] = d * d;
  }
  return sqrt(svm_sum(work, n) / (double)n);
}

/* _shape_error_db, :1446-1465, over a K-bin grid */
static inline double svm_shape_error_db(const double *freqs, const double *db, int K, int preset, svm_offset_scalars *scalars /* nullable */) {
  int first, n;
  double *target, *work, err;
  if (scalars) memset(scalars, 0, sizeof *scalars);
  svm_bin_range(freqs, K, SVM_MASK_LOW, SVM_MASK_HIGH, 1, &first, &n);
  if (n < SVM_MIN_BINS) return INFINITY;
  target = (double *)malloc(sizeof(double) * 3 * (size_t)n);
  work = target + n;
  svm_target_curve(freqs + first, db + first, n, preset, target, scalars, work);
  err = svm_centred_rms(db + first, target, n, work);
  free(target);
  return err;
}

/* :1562-1575: the original's median spectrum interpolated onto the verification's grid, the masked difference less its median,
 * the RMS.  (On one shared grid np.interp returns the original's own values: the kernel reads them directly.)  NaN without a
 * masked bin, as np.mean of nothing. */
static inline double svm_repeatability_delta_db(const double *freqs, const double *before_db, int K, const double *original_freqs,
                                                const double *original_db, int K0) {
  int first, n, i;
  double *delta, *work, m0, out;
  svm_bin_range(freqs, K, SVM_MASK_LOW, SVM_MASK_HIGH, 1, &first, &n);
  if (n == 0) return NAN;
  delta = (double *)malloc(sizeof(double) * 2 * (size_t)n);
  work = delta + n;
  for (i = 0; i < n; ++i) delta[i] = before_db[first + i] - af_interp(freqs[first + i], original_freqs, original_db, K0);
  m0 = svm_median(delta, n, work);
  for (i = 0; i < n; ++i) {
    const double d = delta[i] - m0;
    work[i] = d * d;
  }
  out = sqrt(svm_sum(work, n) / (double)n);
  free(delta);
  return out;
}

/* :1634-1645: low | body | presence | sibilance, lower edge inclusive, upper exclusive; a band without bins is absent */
static const double svm_snr_band_edges[4][2] = {{80.0, 250.0}, {250.0, 1000.0}, {1000.0, 4500.0}, {4500.0, 10000.0}};
static inline void svm_snr_band_medians(const double *freqs, const double *snr_db /* nullable */, int K, double medians[4], int32_t present[4]) {
  double *work = (double *)malloc(sizeof(double) * (size_t)(K > 0 ? K : 1));
  int b;
  for (b = 0; b < 4; ++b) {
    int first = 0, n = 0;
    medians[b] = 0.0;
    present[b] = 0;
    if (!snr_db) continue;
    svm_bin_range(freqs, K, svm_snr_band_edges[b][0], svm_snr_band_edges[b][1], 0, &first, &n);
    if (!n) continue;
    present[b] = 1;
    medians[b] = svm_median(snr_db + first, n, work);
  }
  free(work);
}

/* one signal's levels: the sum of squares, the peak (the largest finite-or-infinite |x|; 0 for an empty signal), whether a
 * sample is not finite, and the two clipped tests, :1490 (>= 0.999) and :1677 (>= 1.0) */
static inline void svm_levels(const float *x, int64_t n, double *sum_squares, double *peak, double *rms_db, int32_t *non_finite,
                              int32_t *clipped_0999, int32_t *clipped_1) {
  double top = 0.0;
  int bad = 0;
  int64_t i;
  for (i = 0; i < n; ++i) {
    const double a = fabs((double)x[i]);
    bad = bad || !isfinite(x[i]);
    if (a > top) top = a;
  }
  *sum_squares = svm_sum_squares(x, n);
  *peak = top;
  *rms_db = svm_rms_db(*sum_squares, n);
  *non_finite = bad;
  *clipped_0999 = top >= 0.999;
  *clipped_1 = top >= 1.0;
}

/* ---- the rules, :1484-1495 and :1590-1679 ---------------------------------------------------------------------------- */
#define SVM_SPEECH_MIN_DURATION_S 3.0 /* SPEECH_MIN_DURATION_S, :43 */
static const char *const svm_reason_texts[AF_SETUP_REASON_COUNT] = {
    "repeatability and native-chain constraints passed",
    "processing is safe but stronger than the selected intensity",
    "candidate chain worsened the target or exceeded a safety limit",
    "verification delivery differs too much from the setup passage",
    "verification passage was too short",
    "verification passage was non-finite or clipped",
    "native verification renderer is unavailable"};

static inline double svm_present(const af_setup_verification_evidence *e, uint32_t bit, double value, double otherwise) {
  return (e->present & bit) ? value : otherwise;
}

static inline void svm_decide(const af_setup_verification_row *row, const af_setup_verification_evidence *e,
                              af_setup_verification_result *o) {
  const int V = AF_SETUP_SIGNAL_VERIFICATION, R = AF_SETUP_SIGNAL_RENDERED;
  memset(o, 0, sizeof *o);
  o->early_exit = 1;
  o->decision = AF_SETUP_RETRY;
  if (e->verification_samples < (int64_t)(e->sample_rate * SVM_SPEECH_MIN_DURATION_S)) { /* :1484, int() truncates */
    o->reason = AF_SETUP_REASON_TOO_SHORT;
    return;
  }
  if (row->non_finite[V] || row->clipped_0999[V]) { /* :1490 */
    o->reason = AF_SETUP_REASON_CLIPPED;
    return;
  }
  if (!e->backend_is_rust) { /* :1527-1537 */
    o->reason = AF_SETUP_REASON_NO_RENDERER;
    return;
  }
  o->early_exit = 0;
  {
    const double target_p95 = svm_present(e, AF_SETUP_HAS_TARGET_P95, e->target_p95_reduction_db, 3.5);
    const double peak_cap = svm_present(e, AF_SETUP_HAS_PEAK_CAP, e->peak_reduction_cap_db, 8.0);
    const double measured_p95 = svm_present(e, AF_SETUP_HAS_COMPRESSOR_P95, e->compressor_gain_reduction_p95_db, 120.0);
    const double measured_peak = svm_present(e, AF_SETUP_HAS_COMPRESSOR_PEAK, e->compressor_gain_reduction_db, 120.0);
    const double output_true_peak = svm_present(e, AF_SETUP_HAS_OUTPUT_TRUE_PEAK, e->output_true_peak_db, 120.0);
    const double ceiling = svm_present(e, AF_SETUP_HAS_CEILING, e->limiter_effective_ceiling_db, -1.5);
    const uint64_t events = (e->present & AF_SETUP_HAS_LIMITED_EVENTS) ? e->true_peak_limited_events : 0;
    const double deesser_p95 = svm_present(e, AF_SETUP_HAS_DEESSER_P95, e->deesser_gain_reduction_p95_db, 0.0);
    const double deesser_max = svm_present(e, AF_SETUP_HAS_DEESSER_MAX_REDUCTION, e->deesser_max_reduction_db, 6.0);
    const double noise_change = row->rms_db[AF_SETUP_SIGNAL_RENDERED_NOISE] - row->rms_db[AF_SETUP_SIGNAL_NOISE]; /* :1600 */
    const double speech_gain = svm_present(e, AF_SETUP_HAS_OUTPUT_RMS, e->output_rms_db, row->rms_db[R]) -
                               svm_present(e, AF_SETUP_HAS_INPUT_RMS, e->input_rms_db, row->rms_db[V]); /* :1601-1603 */
    const double relative = noise_change - speech_gain;
    const double snr_change = e->after_snr_db - e->before_snr_db;
    const double before = row->spectral_target_error_before_db, after = row->spectral_target_error_after_db;
    const double level_difference = row->rms_db[V] - row->rms_db[AF_SETUP_SIGNAL_ORIGINAL];
    if (fabs(level_difference) > 8.0 || row->shape_delta_db > 5.0) { /* :1608 */
      o->decision = AF_SETUP_RETRY;
      o->reason = AF_SETUP_REASON_DIFFERS;
    } else if (after > before + 1.0 || relative > 4.0 || snr_change < -4.0 || measured_peak > peak_cap + 0.25 ||
               output_true_peak > ceiling + 0.15) { /* :1611-1617 */
      o->decision = AF_SETUP_ROLLBACK;
      o->reason = AF_SETUP_REASON_WORSENED;
    } else if (measured_p95 > target_p95 + 0.75 || events > 0 || relative > 3.0 || deesser_p95 > deesser_max * 0.9) { /* :1620-1627 */
      o->decision = AF_SETUP_REDUCE;
      o->reason = AF_SETUP_REASON_STRONGER;
    } else {
      o->decision = AF_SETUP_ACCEPT;
      o->reason = AF_SETUP_REASON_PASSED;
    }
    o->clipped = row->clipped_1[R]; /* :1677 */
    o->limiter_activity_events = events;
    o->spectral_target_error_before_db = before;
    o->spectral_target_error_after_db = after;
    o->loudness_variation_before_db = e->loudness_variation_before_db;
    o->loudness_variation_after_db = e->loudness_variation_after_db;
    o->noise_floor_change_db = noise_change;
    o->relative_noise_floor_change_db = relative;
    o->snr_change_db = snr_change;
    o->compressor_gain_reduction_median_db = svm_present(e, AF_SETUP_HAS_COMPRESSOR_MEDIAN, e->compressor_gain_reduction_median_db, 0.0);
    o->compressor_gain_reduction_p95_db = measured_p95;
    o->compressor_gain_reduction_peak_db = measured_peak;
    o->deesser_gain_reduction_median_db = svm_present(e, AF_SETUP_HAS_DEESSER_MEDIAN, e->deesser_gain_reduction_median_db, 0.0);
    o->deesser_gain_reduction_p95_db = deesser_p95;
    o->output_true_peak_db = output_true_peak;
    o->level_difference_db = level_difference;
    o->shape_delta_db = row->shape_delta_db;
  }
}

/* ---- the offline validation and the confidences, :1265-1364 ------------------------------------------------------------ */
static const char *const svm_uncertainty_texts[AF_SETUP_UNCERTAIN_COUNT] = {
    "too little VAD-active speech", "speech-to-noise ratio is weak", "spectral feature stability is weak",
    "offline DSP validation did not pass", "offline DSP validation is advisory without the Rust extension",
    "Auto-EQ abstained from this capture"};

static inline double svm_clamp(double v, double lo, double hi) { /* _clamp, :82-83: max(low, min(high, value)) */
  const double m = hi < v ? hi : v;
  return lo > m ? lo : m;
}

/* _bounded_quality_score, :86-99: np.sum adds the few terms in index order */
static inline double svm_quality_score(const double *values, const double *weights, int n) {
  double total = 0.0, sum = 0.0;
  int i;
  for (i = 0; i < n; ++i) total += weights[i] > 0.0 ? weights[i] : 0.0;
  if (n <= 0 || total <= 0.0) return 0.0;
  for (i = 0; i < n; ++i) {
    const double w = (weights[i] > 0.0 ? weights[i] : 0.0) / total, v = svm_clip(values[i], 0.0, 1.0);
    sum += w * log(v > 0.03 ? v : 0.03);
  }
  return exp(sum);
}

static inline void svm_offline_validation(const af_setup_offline_inputs *in, af_setup_offline_result *o) {
  const double capture = in->capture_confidence;
  const double dynamics = svm_clamp(in->speech_dynamic_range_db / 8.0, 0.0, 1.0);
  const double quiet_room = svm_clamp((-32.0 - in->conservative_noise_rms_db) / 18.0, 0.0, 1.0);
  double values[5], weights[5] = {0.35, 0.25, 0.15, 0.15, 0.10}, pair_weights[2] = {0.55, 0.45}, setup;
  int passed = 0, weak, eq_apply;
  memset(o, 0, sizeof *o);
  o->eq_confidence = in->has_eq_settings && in->eq_has_analysis_confidence ? in->eq_analysis_confidence : capture; /* :1271 */
  o->gate_confidence = svm_clip(0.55 * capture + 0.45 * in->snr_confidence, 0.0, 1.0);
  values[0] = capture;
  values[1] = in->deesser_frame_evidence_confidence;
  o->deesser_confidence = svm_quality_score(values, pair_weights, 2);
  o->compressor_confidence = svm_clip(0.55 * capture + 0.45 * dynamics, 0.0, 1.0);
  values[0] = o->eq_confidence;
  values[1] = o->gate_confidence;
  values[2] = !in->deesser_enabled && o->deesser_confidence < 0.50 ? 0.50 : o->deesser_confidence; /* :1284 */
  values[3] = o->compressor_confidence;
  values[4] = quiet_room;
  setup = svm_quality_score(values, weights, 5);
  if (in->simulation_available) { /* :1313-1328 */
    const double true_peak = (in->present & AF_SETUP_HAS_OUTPUT_TRUE_PEAK) ? in->output_true_peak_db : 120.0;
    const double ceiling = (in->present & AF_SETUP_HAS_CEILING) ? in->limiter_effective_ceiling_db : -1.5;
    const double peak = (in->present & AF_SETUP_HAS_COMPRESSOR_PEAK) ? in->compressor_gain_reduction_db : 120.0;
    const double p95 = (in->present & AF_SETUP_HAS_COMPRESSOR_P95) ? in->compressor_gain_reduction_p95_db : peak;
    const double deesser = (in->present & AF_SETUP_HAS_DEESSER_PEAK) ? in->deesser_gain_reduction_db : 120.0;
    passed = isfinite(true_peak) && isfinite(peak) && isfinite(deesser) && true_peak <= ceiling + 0.15 &&
             peak <= in->peak_reduction_cap_db + 0.25 && p95 <= in->target_p95_reduction_db + 1.25 && deesser <= 10.0;
  }
  if (in->active_duration_s < 2.0) o->uncertainty_reasons |= AF_SETUP_UNCERTAIN_LITTLE_SPEECH;
  if (in->noise_referenced_snr_db < 8.0) o->uncertainty_reasons |= AF_SETUP_UNCERTAIN_WEAK_SNR;
  if (capture < 0.50) o->uncertainty_reasons |= AF_SETUP_UNCERTAIN_UNSTABLE;
  if (!passed) o->uncertainty_reasons |= AF_SETUP_UNCERTAIN_NOT_PASSED;
  if (!in->backend_is_rust) { /* :1342-1344; the error dict of :1330 reads "unavailable" */
    o->uncertainty_reasons |= AF_SETUP_UNCERTAIN_ADVISORY;
    setup *= 0.90;
  }
  weak = in->active_duration_s < 2.0 || in->noise_referenced_snr_db < 8.0 || capture < 0.50 || !in->noise_status_usable;
  eq_apply = in->has_eq_settings && in->eq_apply_recommended;
  if (!eq_apply) o->uncertainty_reasons |= AF_SETUP_UNCERTAIN_EQ_ABSTAINED;
  if (weak && setup > 0.49) setup = 0.49;
  o->offline_validation_passed = passed;
  o->weak_capture = weak;
  o->apply_recommended = !weak && eq_apply && passed;
  o->setup_confidence = svm_clip(setup, 0.0, 1.0);
  o->recommendation_uncertainty = 1.0 - o->setup_confidence;
}

/* every field of one stream's row; the three spectra share the K-bin grid */
static inline void svm_measure_row(const double *freqs, int K, const double *original_db, const double *before_db, const double *after_db,
                                   const double *after_snr_db /* nullable */, int preset, const float *const audio[AF_SETUP_SIGNALS],
                                   const int64_t lengths[AF_SETUP_SIGNALS], af_setup_verification_row *row) {
  svm_offset_scalars o;
  int first, n, s;
  memset(row, 0, sizeof *row);
  svm_bin_range(freqs, K, SVM_MASK_LOW, SVM_MASK_HIGH, 1, &first, &n);
  row->masked_bins = n;
  row->snr_available = after_snr_db != NULL;
  row->spectral_target_error_before_db = svm_shape_error_db(freqs, before_db, K, preset, &o);
  memcpy(row->offsets_before, &o, sizeof(double) * 5);
  row->spectral_target_error_after_db = svm_shape_error_db(freqs, after_db, K, preset, &o);
  memcpy(row->offsets_after, &o, sizeof(double) * 5);
  row->shape_delta_db = svm_repeatability_delta_db(freqs, before_db, K, freqs, original_db, K);
  svm_snr_band_medians(freqs, after_snr_db, K, row->band_snr_db, row->band_present);
  for (s = 0; s < AF_SETUP_SIGNALS; ++s)
    if (audio[s])
      svm_levels(audio[s], lengths[s], &row->sum_squares[s], &row->peak[s], &row->rms_db[s], &row->non_finite[s],
                 &row->clipped_0999[s], &row->clipped_1[s]);
    else
      row->rms_db[s] = -120.0;
}

#endif
