/* af_speech_features_math.h -- the host half of the speech-feature measurement (python/mic_eq/analysis/voice_setup.py:161-458
 * and deesser_fusion.py:60-78) in f64, on plain arrays: everything that is O(frames) per stream and every log10, exp and
 * percentile.  Plain C so that two readers share one text: af_api_speech_features.cpp between its kernels, and
 * tests/ref/speech_features_ref.c behind its own restatement of those kernels.  What the kernels leave is linear (frame
 * powers, K-weighted chunk energies, band sums, selected middles); the decibels are taken here with the host's libm.
 * Compiled unfused (-ffp-contract=off) on both sides. */
#ifndef AF_SPEECH_FEATURES_MATH_H
#define AF_SPEECH_FEATURES_MATH_H
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/audioforge_mi.h"
#include "af_numpy_rules.h"

#define SFM_RATE 48000          /* the only rate: _k_weighted_48k resamples every other one, :130-132 */
#define SFM_FRAME 1920          /* FRAME_MS 40 */
#define SFM_HOP 960             /* HOP_MS 20 */
#define SFM_VAD_WINDOW 1536     /* ceil(48000 * 512 / 16000), spectrum.py:185-188 */
#define SFM_VAD_EVIDENCE 0.4    /* VAD_SPEECH_EVIDENCE_THRESHOLD, analysis/vad.py */
#define SFM_VAD_STRONG 0.65     /* VAD_STRONG_SPEECH_THRESHOLD */
#define SFM_BAND_FIELDS 8       /* per listed frame: low | body | presence | sibilance | 250-4500 | 5000-9500 | max of the last | 0 */
#define SFM_FEATURES 6          /* FRAME_FEATURE_NAMES, deesser_fusion.py:10-17 */
/* deesser_fusion.py:30-41, the published frame model */
#define SFM_FRAME_INTERCEPT (-14.745480728063148)
static const double sfm_frame_coefficients[SFM_FEATURES] = {1.4074734365324453, 5.220098953258285, 2.427808017651834,
                                                            1.1022350583682425, 4.160012489488813, 2.4617269295476714};

static int sfm_compare(const void *a, const void *b) {
  const double x = *(const double *)a, y = *(const double *)b;
  return (x > y) - (x < y);
}

static inline double sfm_clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }
static inline double sfm_db18(double power) { return 10.0 * log10(power + 1e-18); }
static inline double sfm_lufs(double mean_square) { return -0.691 + 10.0 * log10(mean_square + 1e-12); }

static inline double *sfm_sorted_copy(const double *v, int n) {
  double *s = (double *)malloc(sizeof(double) * (size_t)(n > 0 ? n : 1));
  if (n > 0) memcpy(s, v, sizeof(double) * (size_t)n);
  qsort(s, (size_t)n, sizeof(double), sfm_compare);
  return s;
}

static inline int64_t sfm_frames(int64_t n) { return n < SFM_FRAME ? 0 : (n - SFM_FRAME) / SFM_HOP + 1; }
static inline int64_t sfm_chunks(int64_t n) { return (n + SFM_HOP - 1) / SFM_HOP; } /* the last one may be partial */

/* :178-205 and :269-270 from the frame powers: frame levels, the adaptive floor, the energy mask, the posterior mask with its
 * six-frame rule, the three-frame dilation, and the list of spectrally active frames.  post: [F], written when vad is given. */
static inline void sfm_masks(const double *power, int F, double noise_rms_db, const double *vad, int64_t n_vad, double *frame_db,
                             uint8_t *energy_active, uint8_t *active, double *post, int32_t *listed, af_speech_features_row *r) {
  int f, count = 0, evidence = 0, A = 0, n_active = 0;
  double *sorted, floor_db, p30;
  const int with_vad = vad && n_vad > 0 && F > 0;
  for (f = 0; f < F; ++f) frame_db[f] = 10.0 * log10(power[f] + 1e-12);
  sorted = sfm_sorted_copy(frame_db, F);
  p30 = af_percentile_sorted(sorted, F, 30.0) + 2.0;
  free(sorted);
  floor_db = noise_rms_db + 6.0 > p30 ? noise_rms_db + 6.0 : p30;
  for (f = 0; f < F; ++f) active[f] = energy_active[f] = frame_db[f] >= floor_db;
  if (with_vad) {
    double *xp = (double *)malloc(sizeof(double) * (size_t)n_vad * 2);
    uint8_t *posterior = (uint8_t *)malloc((size_t)F);
    const double low = noise_rms_db + 2.0 > floor_db - 4.0 ? noise_rms_db + 2.0 : floor_db - 4.0;
    af_interpolate_vad_probabilities(vad, n_vad, SFM_VAD_WINDOW, F, SFM_HOP, SFM_FRAME, xp, xp + n_vad, post);
    for (f = 0; f < F; ++f) {
      posterior[f] = (post[f] >= SFM_VAD_EVIDENCE && frame_db[f] >= low) || post[f] >= SFM_VAD_STRONG;
      count += posterior[f];
      evidence += post[f] >= SFM_VAD_EVIDENCE;
    }
    if (count >= 6) memcpy(active, posterior, (size_t)F);
    free(posterior);
    free(xp);
  }
  if (F >= 3) { /* np.convolve(., ones(3), "same") > 0 */
    uint8_t prev = 0;
    for (f = 0; f < F; ++f) {
      const uint8_t here = active[f], next = f + 1 < F ? active[f + 1] : 0;
      active[f] = prev | here | next;
      prev = here;
    }
  }
  for (f = 0; f < F; ++f) {
    n_active += active[f];
    if (active[f] | energy_active[f]) listed[A++] = f;
  }
  r->frames = F;
  r->active_frames = n_active;
  r->spectral_frames = A;
  r->adaptive_floor_db = floor_db;
  r->vad_probability_used = with_vad;
  r->vad_active_frame_ratio = with_vad ? (double)evidence / (double)F : 0.0;
}

/* the loudness values of one window size from the chunk energies, :143-158: windows of `W` chunks every `H`, kept when at
 * least 0.55 of their samples are masked; returns how many, values into out */
static inline int sfm_windows(const double *energy, const uint8_t *chunk_mask, int64_t n, int W, int H, double *out) {
  int count = 0;
  int64_t c0;
  for (c0 = 0; (c0 + W) * SFM_HOP <= n; c0 += H) {
    int masked = 0, c;
    double sum = 0.0;
    for (c = 0; c < W; ++c) masked += chunk_mask[c0 + c];
    if ((double)((int64_t)masked * SFM_HOP) / (double)((int64_t)W * SFM_HOP) < 0.55) continue;
    for (c = 0; c < W; ++c) sum += energy[c0 + c];
    out[count++] = sfm_lufs(sum / (double)((int64_t)W * SFM_HOP));
  }
  return count;
}

/* :207-261: the sample mask on the hop grid (frame f covers chunks f and f + 1; the tail behind the last frame is never
 * masked), duration and ratio, both window sizes with both fallbacks, medians and the spread */
static inline void sfm_loudness(const double *energy /* [sfm_chunks(n)] */, int64_t n, const uint8_t *active, int F,
                                af_speech_features_row *r) {
  const int C = (int)sfm_chunks(n);
  uint8_t *mask = (uint8_t *)calloc((size_t)C + 1, 1);
  double *momentary = (double *)malloc(sizeof(double) * (size_t)(C + 1)), *short_term = (double *)malloc(sizeof(double) * (size_t)(C + 1));
  double *sorted;
  int f, c, n_m, n_s;
  int64_t masked = 0;
  for (f = 0; f < F; ++f)
    if (active[f]) mask[f] = mask[f + 1] = 1;
  for (c = 0; c < C; ++c) masked += mask[c];
  r->active_duration_s = (double)(masked * SFM_HOP) / (double)SFM_RATE;
  r->active_ratio = (double)(masked * SFM_HOP) / (double)n;
  n_m = sfm_windows(energy, mask, n, 20, 5, momentary);    /* 0.400 s every 0.100 s */
  n_s = sfm_windows(energy, mask, n, 150, 50, short_term); /* 3 s every 1 s */
  if (n_m == 0) { /* the mean over the masked samples, :243-249 */
    double sum = 0.0;
    for (c = 0; c < C; ++c)
      if (mask[c]) sum += energy[c];
    momentary[0] = sfm_lufs(masked ? sum / (double)(masked * SFM_HOP) : 0.0);
    n_m = 1;
  }
  if (n_s == 0) {
    memcpy(short_term, momentary, sizeof(double) * (size_t)n_m);
    n_s = n_m;
  }
  sorted = sfm_sorted_copy(momentary, n_m);
  r->momentary_lufs = af_median_sorted(sorted, n_m);
  r->active_loudness_spread_db = n_m >= 4 ? af_percentile_sorted(sorted, n_m, 95.0) - af_percentile_sorted(sorted, n_m, 10.0) : 0.0;
  r->loudness_range_db = r->active_loudness_spread_db;
  free(sorted);
  sorted = sfm_sorted_copy(short_term, n_s);
  r->short_term_lufs = af_median_sorted(sorted, n_s);
  free(sorted);
  r->loudness_window_count = n_m;
  r->short_term_window_count = n_s;
  free(short_term);
  free(momentary);
  free(mask);
}

/* np.median over decibels of a column from its two selected middles (the decibel is monotone, so the median only selects) */
static inline double sfm_median_db18(double lower, double upper) {
  const double lo = sfm_db18(lower), hi = upper == lower ? lo : sfm_db18(upper);
  return (lo + hi) / 2.0;
}

static inline double sfm_sigmoid(double logit) { /* deesser_fusion.py:60-67 */
  if (logit >= 0.0) return 1.0 / (1.0 + exp(-logit));
  {
    const double e = exp(logit);
    return e / (1.0 + e);
  }
}

/* :286-289 and :303-430 up to the weights of the candidate spectrum, for the A listed frames of one stream.
 * band: [A][SFM_BAND_FIELDS] what the frame kernel left; sib_mid: [A][2] the middles of the 5000-9500 Hz bins of each frame;
 * sib_arg: [A] the first arg-max among them; post: the frame posteriors [F] or null; band_mid: [2][SFM_BAND_FIELDS] middles
 * over the listed frames; noise_mid: the two middles of the noise frames' 5000-9500 Hz sums (Fn of them; unused when Fn is 0);
 * sib_freqs: the band's bin frequencies.  Writes features [A][6], probabilities [A], weights [A] = max(p, 1e-6). */
static inline void sfm_evidence(const double *model /* intercept | 6 coefficients */, int A, const int32_t *listed, const double *band,
                                const double *sib_mid, const int32_t *sib_arg, const double *post, const double *band_mid, int Fn,
                                const double *noise_mid, const double *sib_freqs, double *features, double *probabilities,
                                double *weights, af_speech_features_row *r) {
  int i, j;
  r->noise_frames = Fn;
  r->band_low_db = r->band_body_db = r->band_presence_db = r->band_sibilance_db = -120.0;
  r->evidence_available = 0;
  r->confidence = 0.0;
  r->frame_probability_p90 = r->frame_probability_top_mean = r->temporal_score = 0.0;
  r->absolute_hf_strength_p90 = r->noise_reliability_p90 = 0.0;
  r->excess_p90_db = -120.0;
  r->temporal_contrast_db = r->candidate_frame_ratio = r->candidate_snr_db = 0.0;
  r->peak_hz = 6500.0;
  if (A > 0) {
    double *sib = (double *)malloc(sizeof(double) * (size_t)A * 3), *excess = sib + A, *snr = excess + A, *sorted;
    double noise_db, excess_median, excess_p90, contrast, sum = 0.0, dot = 0.0, top = 0.0;
    int top_count;
    r->band_low_db = sfm_median_db18(band_mid[0], band_mid[SFM_BAND_FIELDS + 0]);
    r->band_body_db = sfm_median_db18(band_mid[1], band_mid[SFM_BAND_FIELDS + 1]);
    r->band_presence_db = sfm_median_db18(band_mid[2], band_mid[SFM_BAND_FIELDS + 2]);
    r->band_sibilance_db = sfm_median_db18(band_mid[3], band_mid[SFM_BAND_FIELDS + 3]);
    for (i = 0; i < A; ++i) {
      sib[i] = sfm_db18(band[(size_t)i * SFM_BAND_FIELDS + 5]);
      excess[i] = sib[i] - sfm_db18(band[(size_t)i * SFM_BAND_FIELDS + 4]);
    }
    sorted = sfm_sorted_copy(sib, A);
    noise_db = af_percentile_sorted(sorted, A, 10.0);
    free(sorted);
    if (Fn > 0) noise_db = sfm_median_db18(noise_mid[0], noise_mid[1]);
    sorted = sfm_sorted_copy(excess, A);
    excess_median = af_median_sorted(sorted, A);
    excess_p90 = af_percentile_sorted(sorted, A, 90.0);
    free(sorted);
    contrast = excess_p90 - excess_median > 0.0 ? excess_p90 - excess_median : 0.0;
    for (i = 0; i < A; ++i) {
      double *x = features + (size_t)i * SFM_FEATURES, logit = model[0];
      const double peak = band[(size_t)i * SFM_BAND_FIELDS + 6];
      const double top_db = 10.0 * log10(peak > 1e-18 ? peak : 1e-18);
      const double lo = sib_mid[2 * i] > 1e-18 ? sib_mid[2 * i] : 1e-18, hi = sib_mid[2 * i + 1] > 1e-18 ? sib_mid[2 * i + 1] : 1e-18;
      const double lo_db = 10.0 * log10(lo), mid_db = (lo_db + (hi == lo ? lo_db : 10.0 * log10(hi))) / 2.0;
      const double hz = sib_freqs[sib_arg[i]], octaves = log2((hz > 1.0 ? hz : 1.0) / 6500.0) / 0.70;
      snr[i] = sib[i] - noise_db;
      x[0] = sfm_clip((excess[i] - 0.50) / 5.0, 0.0, 1.0);
      x[1] = sfm_clip((excess[i] - excess_median - 0.20) / 3.0, 0.0, 1.0);
      x[2] = sfm_clip((snr[i] - 3.0) / 15.0, 0.0, 1.0);
      x[3] = post ? 1.0 - sfm_clip(post[listed[i]], 0.0, 1.0) : 0.5;
      x[4] = sfm_clip((top_db - mid_db - 1.0) / 8.0, 0.0, 1.0);
      x[5] = sfm_clip(exp(-0.5 * (octaves * octaves)), 0.0, 1.0);
      for (j = 0; j < SFM_FEATURES; ++j) logit += sfm_clip(x[j], 0.0, 1.0) * model[1 + j];
      probabilities[i] = sfm_sigmoid(logit);
      weights[i] = probabilities[i] > 1e-6 ? probabilities[i] : 1e-6;
      sum += probabilities[i];
      dot += probabilities[i] * snr[i];
    }
    r->candidate_frame_ratio = sum / (double)A;
    r->candidate_snr_db = dot / (sum > 1e-9 ? sum : 1e-9);
    r->temporal_score = sfm_clip((contrast - 0.50) / 2.5, 0.0, 1.0);
    sorted = sfm_sorted_copy(probabilities, A);
    r->frame_probability_p90 = af_percentile_sorted(sorted, A, 90.0);
    top_count = (int)ceil((double)A * 0.10);
    if (top_count < 1) top_count = 1;
    for (i = A - top_count; i < A; ++i) top += sorted[i];
    r->frame_probability_top_mean = top / (double)top_count;
    free(sorted);
    for (j = 0; j < 3; j += 2) { /* the 90th percentiles of feature columns 0 and 2 */
      double *column = (double *)malloc(sizeof(double) * (size_t)A);
      for (i = 0; i < A; ++i) column[i] = features[(size_t)i * SFM_FEATURES + j];
      qsort(column, (size_t)A, sizeof(double), sfm_compare);
      *(j ? &r->noise_reliability_p90 : &r->absolute_hf_strength_p90) = af_percentile_sorted(column, A, 90.0);
      free(column);
    }
    r->evidence_available = 1;
    r->confidence = r->frame_probability_p90;
    r->excess_p90_db = excess_p90;
    r->temporal_contrast_db = contrast;
    free(sib);
  }
  r->sibilance_excess_db = r->band_sibilance_db - r->band_presence_db;
}

#endif
