// af_latency_math.h -- the sum orders and the rules of the latency calibration (python/mic_eq/analysis/latency_calibration.py),
// f64, shared by the kernels of af_latency.hip (which define LM_FN and SVM_FN as host-and-device qualifiers before they include
// this file) and the host half, af_api_latency.cpp.
//
// ORDER OF THE SUMS
//   mean(x), sum(ref * ref)   NumPy's own order, so both are NumPy's bit for bit: buffers of 8192 terms added to a running total,
//                             a buffer by pairwise_sum.  The splitting rule and its constants are af_setup_verification_math.h's
//                             (svm_pairwise_left, SVM_PAIRWISE_*); only the block over plain terms is new here.
//   the energy prefix         np.cumsum(rec * rec): one running f64 sum per stream, sequential.  window_energy is a difference
//                             of two prefix values that cancels in quiet windows; a sum in another order would move those scores
//                             by n u E_total / E_window, far more than the correlation's own rounding.
//   a correlation             sum_k rec[lag + k] ref[k], k ascending, one product and one add per term, from 0.0.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/audioforge_mi.h"
#include "af_numpy_rules.h"
#include "af_setup_verification_math.h"

#ifndef LM_FN
#define LM_FN static inline
#endif

#define LM_MAX_OFFSETS 4      // DEFAULT_REPETITIONS, :21
#define LM_FULL_BIAS 0.985    // :349, :417
#define LM_BURST_BIAS 0.94    // :375
#define LM_SKIP_BELOW 0.035   // :377
#define LM_MIN_PROBE 16       // :279, :326

// one block of NumPy's pairwise sum over plain terms (float32 samples are taken to f64 first)
template <class T>
LM_FN double lm_pairwise_block(const T *a, int64_t n) {
  double r[8], res;
  int64_t i;
  if (n < 8) {
    res = 0.0;
    for (i = 0; i < n; ++i) res += (double)a[i];
    return res;
  }
  for (int j = 0; j < 8; ++j) r[j] = (double)a[j];
  for (i = 8; i < n - (n % 8); i += 8)
    for (int j = 0; j < 8; ++j) r[j] += (double)a[i + j];
  res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += (double)a[i];
  return res;
}

// np.sum over a whole contiguous signal: the walk of svm_pairwise_sum_squares with the block above
template <class T>
LM_FN double lm_sum(const T *a, int64_t n) {
  double total = 0.0;
  for (int64_t at = 0; at < n; at += SVM_PAIRWISE_BUFFER) {
    const T *b = a + at;
    double waiting[SVM_PAIRWISE_DEPTH], value;
    int64_t lo = 0, len = n - at < SVM_PAIRWISE_BUFFER ? n - at : SVM_PAIRWISE_BUFFER, right_len[SVM_PAIRWISE_DEPTH];
    uint64_t went_right = 0;
    int depth = 0;
    for (;;) {
      while (len > SVM_PAIRWISE_BLOCK) {
        const int64_t half = svm_pairwise_left(len);
        right_len[depth] = len - half;
        went_right &= ~((uint64_t)1 << depth);
        len = half;
        ++depth;
      }
      value = lm_pairwise_block(b + lo, len);
      lo += len;
      while (depth > 0 && ((went_right >> (depth - 1)) & 1)) {
        --depth;
        value = waiting[depth] + value;
      }
      if (depth == 0) break;
      waiting[depth - 1] = value;
      went_right |= (uint64_t)1 << (depth - 1);
      len = right_len[depth - 1];
    }
    total += value;
  }
  return total;
}

LM_FN double lm_clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// int(x) of Python for a lag: towards zero, held inside what an int32 lag can be
LM_FN int32_t lm_int(double x) {
  if (!(x > -1.0e9)) return -1000000000;
  if (!(x < 1.0e9)) return 1000000000;
  return (int32_t)x;
}

// _normalized_correlation_scores's last line, :165-167
LM_FN double lm_score(double corr, double window_energy, double ref_energy) {
  return fabs(corr) / sqrt((window_energy > 1e-12 ? window_energy : 1e-12) * ref_energy);
}

// _parabolic_peak_offset, :125-134
LM_FN double lm_parabolic_offset(double left, double center, double right) {
  const double denom = left - 2.0 * center + right;
  if (fabs(denom) < 1e-12) return 0.0;
  return lm_clip(0.5 * (left - right) / denom, -0.5, 0.5);
}

LM_FN int32_t lm_exclusion_radius(int32_t count) {  // :219
  const int32_t r = count / 50 < 128 ? count / 50 : 128;
  return r > 1 ? r : 1;
}

// what one pick leaves, :201-229 (the off-peak median is never read, :346, :372, :414)
typedef struct lm_pick {
  double peak_lag, peak_value, margin, ambiguity;
} lm_pick;

LM_FN lm_pick lm_pick_from(double lag_at_index, double offset, double peak, double second) {
  lm_pick p;
  const double ratio = second / (peak + 1e-6);
  p.peak_lag = lag_at_index + offset;
  p.peak_value = peak;
  p.margin = 1.0 - ratio > 0.0 ? 1.0 - ratio : 0.0;
  p.ambiguity = lm_clip(ratio, 0.0, 1.0);
  return p;
}

// the lag window of one burst, :360-362: Python's round is round-half-even, which rint is in the default rounding mode
LM_FN void lm_burst_window(double coarse_start, int32_t offset, int32_t local_radius, int32_t min_lag, int32_t max_lag,
                           int32_t *lag_min, int32_t *lag_max) {
  const double expected = coarse_start + (double)offset;
  const int32_t a = lm_int(rint(expected - (double)local_radius)), b = lm_int(rint(expected + (double)local_radius));
  const int64_t lo = (int64_t)min_lag + offset, hi = (int64_t)max_lag + offset;
  *lag_min = lo > a ? (int32_t)(lo > 1000000000 ? 1000000000 : lo) : a;
  *lag_max = hi < b ? (int32_t)(hi < -1000000000 ? -1000000000 : hi) : b;
}

// ---- the record one stream leaves on the device, and the host rules over it ------------------------------------------------
typedef struct lm_record {
  int32_t non_finite;                 // a sample of the recording is not finite: nothing below was computed
  int32_t full_count;                 // lags of the whole-probe search
  lm_pick full;
  int32_t burst_count[LM_MAX_OFFSETS];                                   // lags scored per offset, 0: an empty window
  int32_t burst_lo[LM_MAX_OFFSETS];                                      // the first of them
  int32_t lag_min[LM_MAX_OFFSETS], lag_max[LM_MAX_OFFSETS];              // the window of :361-362, before it meets the capture
  int32_t phat_lo[LM_MAX_OFFSETS], phat_count[LM_MAX_OFFSETS];           // the part of it inside (-n/2, n/2]
  int32_t phat_hint[LM_MAX_OFFSETS];
  int32_t reserved[3];
  lm_pick burst[LM_MAX_OFFSETS];
  double mean;
} lm_record;

// the search of one stream, from the keywords of analyze_latency, :290-323
typedef struct lm_search {
  int32_t min_lag, max_lag, expected_window_used, exit_code;
  double playback_min_ms, playback_max_ms, expected_min, expected_max, expected_playback_start_ms;
} lm_search;

static inline lm_search lm_search_from(const af_latency_search *s, double sample_rate, int64_t rec_size, int64_t ref_size) {
  lm_search q = {};
  if (!s->route_supported) { q.exit_code = AF_LATENCY_EXIT_ROUTE; return q; }
  if (rec_size < ref_size) { q.exit_code = AF_LATENCY_EXIT_SHORT; return q; }
  q.min_lag = lm_int((s->min_search_ms / 1000.0) * sample_rate);
  q.max_lag = lm_int((s->max_search_ms / 1000.0) * sample_rate);
  q.expected_window_used = s->has_playback_start != 0;
  q.expected_min = s->has_latency_min ? s->expected_latency_min_ms : s->min_search_ms;
  q.expected_max = s->has_latency_max ? s->expected_latency_max_ms : s->max_search_ms;
  if (q.expected_window_used) {
    const double jitter = s->has_playback_jitter && s->expected_playback_jitter_ms > 0.0 ? s->expected_playback_jitter_ms : 0.0;
    q.expected_playback_start_ms = s->expected_playback_start_ms;
    q.playback_min_ms = std::max(0.0, s->expected_playback_start_ms - jitter);
    q.playback_max_ms = std::max(q.playback_min_ms, s->expected_playback_start_ms + jitter);
    q.min_lag = lm_int(((q.playback_min_ms + q.expected_min) / 1000.0) * sample_rate);
    q.max_lag = lm_int(((q.playback_max_ms + q.expected_max) / 1000.0) * sample_rate);
  }
  if (!(q.max_lag > q.min_lag)) { q.exit_code = AF_LATENCY_EXIT_WINDOW; return q; }
  if (std::min<int64_t>(q.max_lag, rec_size - ref_size) < std::max<int64_t>(q.min_lag, 0)) q.exit_code = AF_LATENCY_EXIT_NO_OVERLAP;
  return q;
}

static inline double lm_median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return af_median_sorted(v.data(), (int)v.size());
}

// analyze_latency:353-515 from the record
static inline void lm_fold(const lm_record &r, const lm_search &q, double sample_rate, int n_offsets, const int32_t *offsets,
                           af_latency_result *out) {
  *out = af_latency_result{};
  out->exit_code = q.exit_code;
  if (q.exit_code != AF_LATENCY_EXIT_NONE) return;
  if (r.non_finite) { out->exit_code = AF_LATENCY_EXIT_NON_FINITE; return; }
  std::vector<double> estimates, peaks{r.full.peak_value}, margins{r.full.margin}, ambiguities{r.full.ambiguity}, phat;
  for (int k = 0; k < n_offsets; ++k) {
    if (r.burst_count[k] <= 0 || r.burst[k].peak_value < LM_SKIP_BELOW) continue;
    const double start = r.burst[k].peak_lag - (double)offsets[k];
    estimates.push_back(start);
    peaks.push_back(r.burst[k].peak_value);
    margins.push_back(r.burst[k].margin);
    ambiguities.push_back(r.burst[k].ambiguity);
    if (r.phat_count[k] > 0) {
      const double phat_start = (double)(r.phat_hint[k] - offsets[k]);
      phat.push_back(std::max(0.0, 1.0 - fabs(phat_start - start) / std::max(1.0, sample_rate * 0.006)));
    }
  }
  if (estimates.empty()) {  // :397-422: the whole-probe pick again
    estimates = {r.full.peak_lag};
    peaks = {r.full.peak_value};
    margins = {r.full.margin};
    ambiguities = {r.full.ambiguity};
  }
  const double median_start = lm_median(estimates);
  std::vector<double> dev;
  for (double e : estimates) dev.push_back(fabs(e - median_start));
  std::sort(dev.begin(), dev.end());
  const double agreement_ms = (af_percentile_sorted(dev.data(), (int)dev.size(), 75.0) * 1000.0) / sample_rate;
  double measured = (median_start * 1000.0) / sample_rate;
  if (q.expected_window_used) measured = std::max(0.0, measured - q.expected_playback_start_ms);
  const double peak_value = lm_median(peaks), margin_ratio = lm_median(margins), ambiguity_score = lm_median(ambiguities);
  const double phat_score = phat.empty() ? 0.5 : lm_median(phat);
  const double strength = lm_clip((peak_value - 0.06) / 0.24, 0.0, 1.0), agreement = lm_clip(1.0 - agreement_ms / 4.0, 0.0, 1.0);
  const double repetition = lm_clip((double)estimates.size() / (double)std::min(3, std::max(1, n_offsets)), 0.0, 1.0);
  const double margin_score = lm_clip(margin_ratio / 0.28, 0.0, 1.0), ambiguity_confidence = lm_clip(1.0 - ambiguity_score, 0.0, 1.0);
  double alignment = 0.0;
  if (q.expected_window_used) {
    const double centre_ms = 0.5 * (q.playback_min_ms + q.playback_max_ms + q.expected_min + q.expected_max);
    const int32_t centre = lm_int((centre_ms / 1000.0) * sample_rate);
    const int32_t half_width = std::max(1, (q.max_lag - q.min_lag) / 2);
    alignment = std::max(0.0, 1.0 - (fabs(median_start - (double)centre) / (double)half_width));
  }
  double confidence = 0.24 * strength + 0.24 * agreement + 0.18 * repetition + 0.14 * margin_score + 0.12 * ambiguity_confidence +
                      0.08 * phat_score;
  if (q.expected_window_used) confidence = 0.88 * confidence + 0.12 * alignment;
  const int n_est = (int)estimates.size();
  const bool success = confidence >= 0.32 && measured > 0.0 && peak_value >= 0.07 && ambiguity_score < 0.90 &&
                       n_est >= std::min(2, n_offsets) && agreement_ms <= 6.0;
  out->success = success;
  out->message = success ? AF_LATENCY_MESSAGE_OK
                 : (agreement_ms > 6.0 && n_est > 1) ? AF_LATENCY_MESSAGE_DISAGREE
                 : ambiguity_score > 0.82 ? AF_LATENCY_MESSAGE_ECHO
                                          : AF_LATENCY_MESSAGE_LOW_CONFIDENCE;
  out->measured_round_trip_ms = out->applied_compensation_ms = out->route_latency_ms = measured;
  out->confidence = confidence;
  out->peak_sample_offset = (int64_t)rint(median_start);
  out->repetition_count = n_est;
  out->agreement_ms = agreement_ms;
  out->ambiguity_score = ambiguity_score;
  out->sub_sample_offset = median_start;
}
