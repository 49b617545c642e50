/* af_voice_setup_math.h -- the rules of python/mic_eq/analysis/voice_setup.py:1143-1223 and :468-696 in f64 on plain arrays:
 * level percentiles, capture confidence, and the gate, de-esser and compressor recommendations.  Plain C, shared by
 * af_api_voice_setup.cpp and tests/ref/speech_features_ref.c (see af_speech_features_math.h).  Sums run in index order. */
#ifndef AF_VOICE_SETUP_MATH_H
#define AF_VOICE_SETUP_MATH_H
#include "af_speech_features_math.h"

/* deesser_fusion.py:43-57, the published clip model */
#define VSM_CLIP_INTERCEPT (-5.98947017317317)
#define VSM_ENABLE_PROBABILITY_THRESHOLD 0.4935253581578833
static const double vsm_clip_coefficients[6] = {2.9145233318588595, 2.038737680696125, 0.5664410938494544,
                                                0.8808711007448764, 3.440954995939097,  0.8326905545571951};
/* DYNAMICS_PROFILES, :60-79: target_p95_db | target_median_db | peak_cap_db | ratio_scale of gentle, balanced, dense */
static const double vsm_profiles[3][4] = {{2.0, 0.7, 6.0, 0.82}, {3.5, 1.4, 8.0, 1.0}, {5.5, 2.5, 10.0, 1.22}};

static inline double vsm_clamp(double v, double lo, double hi) { /* _clamp, :82-83: max(low, min(high, value)) */
  const double m = hi < v ? hi : v;
  return lo > m ? lo : m;
}

/* _bounded_quality_score, :86-99: the weighted geometric mean of values clipped to [0.03, 1], in the order given */
static inline double vsm_quality_score(const double *values, const double *weights, int n) {
  double total = 0.0, sum = 0.0;
  int i;
  for (i = 0; i < n; ++i) total += weights[i] > 0.0 ? weights[i] : 0.0;
  if (n <= 0 || total <= 0.0) return 0.0;
  for (i = 0; i < n; ++i) {
    const double w = (weights[i] > 0.0 ? weights[i] : 0.0) / total, v = sfm_clip(values[i], 0.0, 1.0);
    sum += w * log(v > 0.03 ? v : 0.03);
  }
  return exp(sum);
}

static inline double vsm_band_mean(const double *freqs, const double *db, int K, double low, double high) { /* _band_mean, :461-465 */
  double sum = 0.0, all = 0.0;
  int k, n = 0;
  for (k = 0; k < K; ++k) {
    all += db[k];
    if (freqs[k] >= low && freqs[k] <= high) { sum += db[k]; ++n; }
  }
  return n ? sum / (double)n : all / (double)K;
}

static inline void vsm_default_inputs(af_voice_setup_inputs *in) {
  memset(in, 0, sizeof *in);
  in->vad_available = 1;
  in->target_lufs = -16.0;
  in->dynamics_intensity = AF_DYNAMICS_BALANCED;
  in->custom_target_p95_db = 3.5;
  in->custom_peak_cap_db = 8.0;
  in->noise_quality_score = 1.0;
  in->enable_probability_threshold = VSM_ENABLE_PROBABILITY_THRESHOLD;
}

static inline void vsm_recommend(const af_voice_setup_inputs *in, af_voice_setup_recommendation *o) {
  const af_speech_features_row *f = in->features;
  const int F = f->frames;
  const double noise_db = in->conservative_noise_rms_db;
  double *levels = (double *)malloc(sizeof(double) * (size_t)(F > 0 ? F : 1));
  int i, n = 0;
  memset(o, 0, sizeof *o);

  /* :1143-1153 */
  for (i = 0; i < F; ++i)
    if (in->active_frame_mask[i]) levels[n++] = in->frame_db[i];
  if (n < 6) {
    memcpy(levels, in->frame_db, sizeof(double) * (size_t)F);
    n = F;
  }
  qsort(levels, (size_t)n, sizeof(double), sfm_compare);
  o->speech_floor_db = af_percentile_sorted(levels, n, 20.0);
  o->speech_body_db = af_percentile_sorted(levels, n, 60.0);
  o->speech_frame_peak_db = af_percentile_sorted(levels, n, 95.0);
  free(levels);
  o->speech_snr_db = o->speech_body_db - noise_db;

  { /* :1167-1190 */
    double values[5], weights[5] = {0.30, 0.22, 0.23, 0.17, 0.08}, c;
    o->snr_confidence = vsm_clamp((in->snr_db - 6.0) / 12.0, 0.0, 1.0);
    values[0] = in->residual_confidence;
    values[1] = o->snr_confidence;
    values[2] = in->noise_quality_score;
    values[3] = vsm_clamp(f->active_duration_s / 3.0, 0.0, 1.0);
    values[4] = vsm_clamp((double)f->loudness_window_count / 8.0, 0.0, 1.0);
    c = vsm_quality_score(values, weights, 5);
    if (in->snr_db < 6.0 && c > 0.40) c = 0.40;
    if (f->active_duration_s < 2.0 && c > 0.45) c = 0.45;
    if (in->used_single_spectrum_fallback && c > 0.40) c = 0.40;
    if (in->noise_status == AF_NOISE_STATUS_QUESTIONABLE && c > 0.49) c = 0.49;
    else if (in->noise_status == AF_NOISE_STATUS_INVALID && c > 0.20) c = 0.20;
    o->capture_confidence = c;
  }

  { /* _recommend_gate_settings, :468-502 */
    const double gap = -22.0 - o->speech_body_db > 0.0 ? -22.0 - o->speech_body_db : 0.0;
    o->gate_margin_db = vsm_clamp(o->speech_floor_db - noise_db - 3.0, 4.0, 12.0);
    o->gate_threshold_db = vsm_clamp(noise_db + o->gate_margin_db, -80.0, -10.0);
    o->gate_vad_threshold = vsm_clamp(0.46 - (o->speech_snr_db - 10.0) / 800.0, 0.42, 0.50);
    o->gate_vad_pre_gain = vsm_clamp(pow(10.0, gap / 20.0), 1.0, 3.0);
    o->gate_vad_hold_time_ms = vsm_clamp(140.0 + f->loudness_range_db * 6.0, 140.0, 260.0);
    o->gate_mode = in->vad_available ? 1 : 0;
    o->gate_auto_threshold_enabled = in->vad_available ? 1 : 0;
  }

  { /* _recommend_deesser_settings, :505-624 */
    const int K = in->bins, available = f->evidence_available != 0;
    const double presence = vsm_band_mean(in->freqs, in->spectrum_db, K, 2500.0, 4500.0);
    const double sibilance = vsm_band_mean(in->freqs, in->spectrum_db, K, 5000.0, 9000.0);
    const double aggregate = 0.35 * (sibilance - presence) + 0.65 * f->sibilance_excess_db;
    double peak_hz = 6500.0, top = 0.0, excess, p = 0.0, logit = VSM_CLIP_INTERCEPT, *x = o->deesser_clip_features;
    int k, seen = 0, finite = 1;
    for (k = 0; k < K; ++k) /* the first arg-max over 4500-9500 Hz */
      if (in->freqs[k] >= 4500.0 && in->freqs[k] <= 9500.0 && (!seen || in->spectrum_db[k] > top)) {
        top = in->spectrum_db[k];
        peak_hz = in->freqs[k];
        seen = 1;
      }
    excess = available ? f->excess_p90_db : aggregate;
    if (available) peak_hz = f->peak_hz;
    x[0] = available ? f->frame_probability_p90 : 0.0;
    x[1] = available ? f->frame_probability_top_mean : 0.0;
    x[2] = f->candidate_frame_ratio;
    x[3] = available ? f->temporal_score : 0.0;
    x[4] = available ? f->absolute_hf_strength_p90 : 0.0;
    x[5] = available ? f->noise_reliability_p90 : 0.0;
    for (k = 0; k < 6; ++k) finite = finite && isfinite(x[k]);
    if (available) {
      double values[3], weights[3] = {0.70, 0.20, 0.10};
      for (k = 0; k < 6; ++k) logit += sfm_clip(x[k], 0.0, 1.0) * vsm_clip_coefficients[k]; /* predict_clip_probability */
      p = sfm_sigmoid(logit);
      values[0] = p;
      values[1] = in->noise_quality_score;
      values[2] = o->capture_confidence;
      o->deesser_frame_evidence_confidence = vsm_quality_score(values, weights, 3);
    }
    o->deesser_frame_evidence_available = available;
    o->deesser_invalid_evidence = !available || in->noise_status == AF_NOISE_STATUS_INVALID || !finite;
    o->deesser_detection_probability = p;
    o->deesser_enabled = !o->deesser_invalid_evidence && p >= in->enable_probability_threshold;
    o->deesser_auto_amount = vsm_clamp(0.18 + 0.55 * p + 0.12 * vsm_clamp(excess / 6.0, 0.0, 1.0), 0.20, 0.85);
    o->deesser_low_cut_hz = vsm_clamp(peak_hz - 1700.0, 3500.0, 7000.0);
    o->deesser_high_cut_hz = vsm_clamp(peak_hz + 2100.0, o->deesser_low_cut_hz + 1500.0, 11000.0);
    o->deesser_ratio = vsm_clamp(2.5 + (excess > 0.0 ? excess : 0.0) * 0.45, 2.0, 5.5);
    o->deesser_max_reduction_db = vsm_clamp(3.5 + (excess > 0.0 ? excess : 0.0) * 0.65, 3.0, 8.0);
    o->deesser_sibilance_excess_db = excess;
    o->deesser_peak_hz = peak_hz;
  }

  { /* _recommend_compressor_settings, :627-696 */
    const double range = f->loudness_range_db;
    double profile[4];
    int which = in->dynamics_intensity;
    if (which == AF_DYNAMICS_CUSTOM) {
      const double p95 = vsm_clamp(in->custom_target_p95_db, 1.0, 8.0);
      profile[0] = p95;
      profile[1] = vsm_clamp(p95 * 0.42, 0.3, 4.0);
      profile[2] = vsm_clamp(in->custom_peak_cap_db, p95 + 0.5, 12.0);
      profile[3] = vsm_clamp(0.72 + p95 / 12.5, 0.8, 1.35);
    } else {
      if (which < AF_DYNAMICS_GENTLE || which > AF_DYNAMICS_DENSE) which = AF_DYNAMICS_BALANCED;
      memcpy(profile, vsm_profiles[which], sizeof profile);
    }
    o->compressor_profile = which;
    o->compressor_target_lufs = in->target_lufs;
    o->compressor_threshold_db = vsm_clamp(o->speech_body_db - 5.5, -48.0, -14.0);
    o->compressor_ratio = vsm_clamp((2.2 + range / 5.0) * profile[3], 1.8, 5.5);
    o->compressor_attack_ms = vsm_clamp(11.0 - range / 2.5, 4.0, 12.0);
    o->compressor_release_ms = vsm_clamp(135.0 + range * 11.0, 120.0, 260.0);
    o->compressor_base_release_ms = vsm_clamp(50.0 + range * 6.0, 50.0, 140.0);
    o->compressor_auto_makeup_enabled = o->capture_confidence >= 0.55 && o->speech_snr_db >= 10.0;
    o->compressor_makeup_gain_db = o->compressor_auto_makeup_enabled ? 0.0 : vsm_clamp(in->target_lufs - f->short_term_lufs, 0.0, 6.0);
    o->compressor_target_p95_db = profile[0];
    o->compressor_target_median_db = profile[1];
    o->compressor_peak_cap_db = profile[2];
    o->compressor_noise_reference_reliability = sfm_clip(in->noise_quality_score, 0.0, 1.0);
  }
}

#endif
