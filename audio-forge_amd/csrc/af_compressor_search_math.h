/* af_compressor_search_math.h -- the host's share of the compressor candidate sweep, plain C: what is O(blocks) per CAPTURE and
 * the same for every candidate of it (python_api.rs:578-648 as mic_eq_core.chain_diagnostics restates it): the per-block input
 * level in dB, its 20 % / 90 % percentiles, active_analysis_threshold_db and the `active` / `audible` masks.  Computed once here
 * and uploaded, so that both masks carry one libm's bits for every lane.  No HIP, no allocation: the caller brings the arrays. */
#ifndef AF_COMPRESSOR_SEARCH_MATH_H
#define AF_COMPRESSOR_SEARCH_MATH_H
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CSM_MASK_ACTIVE 1
#define CSM_MASK_AUDIBLE 2

/* python_api.rs:54-56 in f32; the logarithm in f64 and rounded once, as the fold kernel takes it (af_compressor_search.hip) */
static inline float csm_linear_to_db(float v) { return 20.0f * (float)log10((double)fmaxf(v, 1.0e-12f)); }

static inline int csm_compare_f32(const void *a, const void *b) {
  const float x = *(const float *)a, y = *(const float *)b;
  return (x > y) - (x < y);
}

/* python_api.rs:58-74 over SORTED values: position in f32, floor and ceil, f32 lerp */
static inline float csm_percentile_sorted(const float *sorted, int n, float pct) {
  if (n <= 0) return 0.0f;
  const float position = (float)(n - 1) * pct;
  const int lo = (int)floorf(position), hi = (int)ceilf(position);
  if (lo == hi) return sorted[lo];
  const float fraction = position - (float)lo;
  return sorted[lo] + fraction * (sorted[hi] - sorted[lo]);
}

/* samples of control block `i` of a capture of n samples */
static inline int csm_block_length(int64_t n, int control_block, int i) {
  const int64_t left = n - (int64_t)i * control_block;
  return (int)(left < control_block ? left : control_block);
}

/* One capture.  input_square_sum: [n_blocks] with `stride` doubles between blocks.  Writes in_db[n_blocks], mask[n_blocks]
 * (CSM_MASK_*); `scratch` holds n_blocks floats.  Returns the number of active blocks. */
static inline int csm_capture_masks(const double *input_square_sum, int64_t stride, int n_blocks, int64_t n_samples, int control_block,
                                    float *in_db, uint8_t *mask, float *scratch, float *active_threshold_db) {
  for (int i = 0; i < n_blocks; ++i) {
    const float rms = (float)sqrt(input_square_sum[(int64_t)i * stride] / (double)csm_block_length(n_samples, control_block, i));
    in_db[i] = csm_linear_to_db(rms);
    scratch[i] = in_db[i];
  }
  qsort(scratch, (size_t)n_blocks, sizeof(float), csm_compare_f32);
  const float floor_db = csm_percentile_sorted(scratch, n_blocks, 0.20f);
  const float p90_db = csm_percentile_sorted(scratch, n_blocks, 0.90f);
  const float threshold = fmaxf(fmaxf(floor_db + 6.0f, p90_db - 24.0f), -60.0f);
  int active = 0;
  for (int i = 0; i < n_blocks; ++i) {
    mask[i] = (uint8_t)((in_db[i] >= threshold ? CSM_MASK_ACTIVE : 0) | (in_db[i] > -100.0f ? CSM_MASK_AUDIBLE : 0));
    active += in_db[i] >= threshold;
  }
  *active_threshold_db = threshold;
  return active;
}

/* the two f32 smoothing factors of the pumping score at a cadence in Hz, python_api.rs:82-87 */
static inline void csm_pumping_alphas(float cadence_hz, float *highpass_alpha, float *lowpass_alpha) {
  const float pi = 3.14159265358979323846f;
  const float dt = 1.0f / cadence_hz;
  const float highpass_rc = 1.0f / (2.0f * pi * 2.0f);
  const float lowpass_rc = 1.0f / (2.0f * pi * 8.0f);
  *highpass_alpha = highpass_rc / (highpass_rc + dt);
  *lowpass_alpha = dt / (lowpass_rc + dt);
}

/* ---- the fold of one simulation's block rows, python_api.rs:578-713: what cs_fold_kernel (af_compressor_search.hip) computes
 * per lane, on the host.  The library folds on the device; this is the same arithmetic for a CPU check on given rows. */
typedef struct csm_fold_rows { /* [n_blocks] each */
  const double *input_square_sum, *output_square_sum;
  const float *input_sample_peak, *output_sample_peak, *tp_limiter_input_peak, *output_true_peak;
  const float *limiter_gr_db, *tp_limiter_gr_db, *compressor_gr_db, *deesser_gr_db;
  const uint32_t *tp_limited_events, *non_finite_output;
} csm_fold_rows;

typedef struct csm_fold_result { /* the numeric keys of python_api.rs:649-712, in their order */
  float input_sample_peak_db, input_rms_db, output_sample_peak_db, pre_limiter_true_peak_db, output_true_peak_db, output_rms_db;
  float limiter_effective_ceiling_db, sample_headroom_db, pre_limiter_true_peak_headroom_db, true_peak_headroom_db;
  float limiter_gain_reduction_db, true_peak_limiter_gain_reduction_db, compressor_gain_reduction_db, deesser_gain_reduction_db;
  float compressor_gain_reduction_median_db, compressor_gain_reduction_p95_db, compressor_gain_reduction_active_ratio;
  float active_output_gain_db, silence_output_gain_db, silence_level_delta_db, compressor_pumping_score_db;
  float deesser_gain_reduction_median_db, deesser_gain_reduction_p95_db, active_analysis_threshold_db;
  int32_t true_peak_limited_events, non_finite_output, active_analysis_block_count, reserved;
} csm_fold_result;

/* percentile of the values whose keep byte is set; `sorted` holds n floats */
static inline float csm_percentile_kept(const float *v, const uint8_t *keep, int n, float pct, float *sorted) {
  int m = 0;
  for (int i = 0; i < n; ++i)
    if (!keep || keep[i]) sorted[m++] = v[i];
  qsort(sorted, (size_t)m, sizeof(float), csm_compare_f32);
  return csm_percentile_sorted(sorted, m, pct);
}

/* python_api.rs:76-111 */
static inline float csm_pumping_score(const float *trace, int n, float cadence_hz, float *bandpass_abs, float *deltas, float *sorted) {
  if (n < 3) return 0.0f;
  float highpass_alpha, lowpass_alpha;
  csm_pumping_alphas(cadence_hz, &highpass_alpha, &lowpass_alpha);
  float previous = trace[0], highpass = 0.0f, bandpass = 0.0f;
  for (int i = 1; i < n; ++i) {
    const float value = trace[i];
    if (!isfinite(value)) return INFINITY;
    highpass = highpass_alpha * (highpass + value - previous);
    bandpass = bandpass + lowpass_alpha * (highpass - bandpass);
    bandpass_abs[i - 1] = fabsf(bandpass);
    deltas[i - 1] = fabsf(value - previous);
    previous = value;
  }
  const float robust_limit = csm_percentile_kept(bandpass_abs, NULL, n - 1, 0.95f, sorted);
  float total = 0.0f;
  for (int i = 0; i < n - 1; ++i) {
    const float v = fminf(bandpass_abs[i], robust_limit);
    total = total + v * v;
  }
  return sqrtf(total / (float)(n - 1)) + csm_percentile_kept(deltas, NULL, n - 1, 0.95f, sorted);
}

/* `scratch`: 6 n_blocks floats, `bytes`: 2 n_blocks bytes */
static inline void csm_fold(const csm_fold_rows *r, int n, int64_t n_samples, int control_block, float ceiling_db, csm_fold_result *out,
                            float *scratch, uint8_t *bytes) {
  float *in_db = scratch, *gain = scratch + n, *comp = scratch + 2 * n, *work = scratch + 3 * n, *sorted = scratch + 4 * n, *more = scratch + 5 * n;
  uint8_t *mask = bytes, *keep = bytes + n;
  csm_fold_result o;
  memset(&o, 0, sizeof o);
  o.active_analysis_block_count = csm_capture_masks(r->input_square_sum, 1, n, n_samples, control_block, in_db, mask, sorted, &o.active_analysis_threshold_db);
  const int use_all = o.active_analysis_block_count < 3; /* python_api.rs:618-625 */
  if (use_all) o.active_analysis_block_count = n;
  double in_total = 0.0, out_total = 0.0;
  float in_peak = 0.0f, out_peak = 0.0f, tp_in_peak = 0.0f, out_tp = 0.0f;
  int above = 0;
  for (int i = 0; i < n; ++i) {
    in_total += r->input_square_sum[i];
    out_total += r->output_square_sum[i];
    in_peak = fmaxf(in_peak, r->input_sample_peak[i]);
    out_peak = fmaxf(out_peak, r->output_sample_peak[i]);
    tp_in_peak = fmaxf(tp_in_peak, r->tp_limiter_input_peak[i]);
    out_tp = fmaxf(out_tp, r->output_true_peak[i]);
    o.limiter_gain_reduction_db = fmaxf(o.limiter_gain_reduction_db, r->limiter_gr_db[i]);
    o.true_peak_limiter_gain_reduction_db = fmaxf(o.true_peak_limiter_gain_reduction_db, r->tp_limiter_gr_db[i]);
    o.compressor_gain_reduction_db = fmaxf(o.compressor_gain_reduction_db, r->compressor_gr_db[i]);
    o.deesser_gain_reduction_db = fmaxf(o.deesser_gain_reduction_db, r->deesser_gr_db[i]);
    o.true_peak_limited_events += (int32_t)r->tp_limited_events[i];
    o.non_finite_output |= r->non_finite_output[i] != 0;
    const float rms = (float)sqrt(r->output_square_sum[i] / (double)csm_block_length(n_samples, control_block, i));
    gain[i] = csm_linear_to_db(rms) - in_db[i];
    comp[i] = r->compressor_gr_db[i] > 0.0f ? r->compressor_gr_db[i] : 0.0f;
    keep[i] = (uint8_t)(use_all || (mask[i] & CSM_MASK_ACTIVE));
    above += keep[i] && comp[i] >= 0.10f;
  }
  const float input_rms = n_samples > 0 ? (float)sqrt(in_total / (double)n_samples) : 0.0f;
  const float output_rms = n_samples > 0 ? (float)sqrt(out_total / (double)n_samples) : 0.0f;
  o.input_sample_peak_db = csm_linear_to_db(in_peak);
  o.input_rms_db = csm_linear_to_db(input_rms);
  o.output_sample_peak_db = csm_linear_to_db(out_peak);
  o.pre_limiter_true_peak_db = csm_linear_to_db(tp_in_peak);
  o.output_true_peak_db = csm_linear_to_db(out_tp);
  o.output_rms_db = csm_linear_to_db(output_rms);
  o.limiter_effective_ceiling_db = ceiling_db;
  o.sample_headroom_db = ceiling_db - o.output_sample_peak_db;
  o.pre_limiter_true_peak_headroom_db = ceiling_db - o.pre_limiter_true_peak_db;
  o.true_peak_headroom_db = ceiling_db - o.output_true_peak_db;
  o.compressor_gain_reduction_median_db = csm_percentile_kept(comp, keep, n, 0.50f, sorted);
  o.compressor_gain_reduction_p95_db = csm_percentile_kept(comp, keep, n, 0.95f, sorted);
  o.compressor_gain_reduction_active_ratio = o.active_analysis_block_count > 0 ? (float)above / (float)o.active_analysis_block_count : 0.0f;
  for (int i = 0; i < n; ++i) work[i] = r->deesser_gr_db[i] > 0.0f ? r->deesser_gr_db[i] : 0.0f;
  o.deesser_gain_reduction_median_db = csm_percentile_kept(work, keep, n, 0.50f, sorted);
  o.deesser_gain_reduction_p95_db = csm_percentile_kept(work, keep, n, 0.95f, sorted);
  for (int i = 0; i < n; ++i) keep[i] = (mask[i] & (CSM_MASK_ACTIVE | CSM_MASK_AUDIBLE)) == (CSM_MASK_ACTIVE | CSM_MASK_AUDIBLE);
  o.active_output_gain_db = csm_percentile_kept(gain, keep, n, 0.50f, sorted);
  for (int i = 0; i < n; ++i) keep[i] = (mask[i] & (CSM_MASK_ACTIVE | CSM_MASK_AUDIBLE)) == CSM_MASK_AUDIBLE;
  o.silence_level_delta_db = csm_percentile_kept(gain, keep, n, 0.50f, sorted);
  for (int i = 0; i < n; ++i) {
    keep[i] = !(mask[i] & CSM_MASK_ACTIVE);
    work[i] = -comp[i];
  }
  o.silence_output_gain_db = csm_percentile_kept(work, keep, n, 0.50f, sorted);
  o.compressor_pumping_score_db = csm_pumping_score(comp, n, 50.0f, work, more, sorted);
  *out = o;
}

/* ---- the calibration search, python/mic_eq/analysis/voice_setup.py:699-1079, in f64 -------------------------------------
 * The reference evaluates one candidate at a time; whether a candidate is evaluated (budget, duplicate key) never depends on a
 * simulation's result, so the candidates of a phase are listed first (csm_phase1 / csm_phase2), simulated as one batch by the
 * caller, and scored in the listed order (csm_score).  Controls are indexed threshold_db, ratio, attack_ms, release_ms. */
#define CSM_BUDGET 68                    /* _COMPRESSOR_SEARCH_BUDGET, :699 */
#define CSM_MAX_EVALUATED (CSM_BUDGET - 1) /* :783 */
#define CSM_CONTROLS 4

static const double csm_bounds[CSM_CONTROLS][2] = {{-55.0, -6.0}, {1.5, 6.0}, {3.0, 25.0}, {60.0, 320.0}}; /* :700-705 */
static const double csm_local_steps[CSM_CONTROLS] = {3.0, 0.5, 3.0, 25.0};                                 /* :937-942 */

typedef struct csm_settings {
  double compressor[CSM_CONTROLS]; /* the settings' own values, not clamped */
  int auto_makeup_enabled;
  double target_lufs, measured_short_term_lufs; /* .get(..., -18.0) each, :833-838 */
  double target_p95_db, target_median_db, peak_cap_db;
} csm_settings;

/* what evaluate() reads of a simulation, :824-847 (f32 results widened to f64, as Python's float() does) */
typedef struct csm_simulation {
  double peak, median, p95, active_ratio, active_gain, output_true_peak, ceiling, pre_limiter_headroom, pumping, silence_gain;
  int non_finite;
} csm_simulation;

typedef struct csm_entry {
  double key[CSM_CONTROLS];       /* key_for(candidate_values): round(x, 6) of the UNCLAMPED candidate, the dict's key */
  double values[CSM_CONTROLS];    /* the clamped candidate: what is simulated and stored, :913 */
  double value_key[CSM_CONTROLS]; /* key_for(values): the sort's tie-break, :930 */
  double score;
} csm_entry;

typedef struct csm_search {
  csm_settings settings;
  double incumbent[CSM_CONTROLS];
  csm_entry entries[CSM_MAX_EVALUATED]; /* `evaluated`, in insertion order */
  int n, n_scored;
} csm_search;

typedef struct csm_choice {
  int feasible;          /* 0: no feasible candidate, the settings stay */
  int best, expanded, threshold_only; /* entries; threshold_only -1 when there is none */
  int expanded_selected;
  double threshold_only_objective, incumbent_objective;
} csm_choice;

static inline double csm_clamp(double v, double lo, double hi) { return fmax(lo, fmin(hi, v)); }

/* Python's round(x, 6): the exact binary value rounded to six decimals, read back */
static inline double csm_round6(double x) {
  char text[64];
  if (!isfinite(x)) return x;
  snprintf(text, sizeof text, "%.6f", x);
  return strtod(text, NULL);
}

static inline double csm_huber(double value) { /* :727-729 */
  const double magnitude = fabs(value);
  return magnitude <= 1.0 ? 0.5 * magnitude * magnitude : magnitude - 0.5;
}

static inline double csm_halton(int index, int base) { /* :732-739 */
  double result = 0.0, scale = 1.0;
  while (index > 0) {
    scale /= base;
    result += scale * (index % base);
    index /= base;
  }
  return result;
}

static inline void csm_begin(csm_search *s, const csm_settings *settings) {
  memset(s, 0, sizeof *s);
  s->settings = *settings;
  for (int k = 0; k < CSM_CONTROLS; ++k) s->incumbent[k] = csm_clamp(settings->compressor[k], csm_bounds[k][0], csm_bounds[k][1]);
}

/* the head of evaluate(), :783-797: budget, duplicate key, clamp.  Returns 1 when the candidate was listed. */
static inline int csm_offer(csm_search *s, const double candidate[CSM_CONTROLS]) {
  if (s->n >= CSM_MAX_EVALUATED) return 0;
  double key[CSM_CONTROLS];
  for (int k = 0; k < CSM_CONTROLS; ++k) key[k] = csm_round6(candidate[k]);
  for (int i = 0; i < s->n; ++i)
    if (s->entries[i].key[0] == key[0] && s->entries[i].key[1] == key[1] && s->entries[i].key[2] == key[2] && s->entries[i].key[3] == key[3])
      return 0;
  csm_entry *e = &s->entries[s->n++];
  for (int k = 0; k < CSM_CONTROLS; ++k) {
    e->key[k] = key[k];
    e->values[k] = csm_clamp(candidate[k], csm_bounds[k][0], csm_bounds[k][1]);
    e->value_key[k] = csm_round6(e->values[k]);
  }
  e->score = INFINITY;
  return 1;
}

/* :916-926.  Returns how many entries wait for a simulation: entries[n_scored .. n). */
static inline int csm_phase1(csm_search *s) {
  double candidate[CSM_CONTROLS];
  csm_offer(s, s->incumbent);
  for (int i = 0; i < 33; ++i) { /* np.linspace(-55.0, -6.0, 33): start + i * step, the last one the stop itself */
    memcpy(candidate, s->incumbent, sizeof candidate);
    candidate[0] = i == 32 ? -6.0 : -55.0 + (double)i * ((-6.0 - -55.0) / 32.0);
    csm_offer(s, candidate);
  }
  static const int bases[CSM_CONTROLS] = {2, 3, 5, 7};
  for (int index = 1; index < 17; ++index) {
    for (int k = 0; k < CSM_CONTROLS; ++k)
      candidate[k] = csm_bounds[k][0] + csm_halton(index, bases[k]) * (csm_bounds[k][1] - csm_bounds[k][0]);
    csm_offer(s, candidate);
  }
  return s->n - s->n_scored;
}

/* the body of evaluate(), :824-914, for the next unscored entry */
static inline void csm_score(csm_search *s, const csm_simulation *sim) {
  csm_entry *e = &s->entries[s->n_scored++];
  const csm_settings *c = &s->settings;
  const double output_lufs = c->auto_makeup_enabled ? c->target_lufs : c->measured_short_term_lufs + sim->active_gain;
  const double finite_values[9] = {sim->peak, sim->median, sim->p95, sim->active_ratio, output_lufs, sim->output_true_peak,
                                   sim->pre_limiter_headroom, sim->pumping, sim->silence_gain};
  int all_finite = 1;
  for (int i = 0; i < 9; ++i) all_finite &= isfinite(finite_values[i]) ? 1 : 0;
  const int hard_rejected = sim->non_finite || !all_finite || sim->output_true_peak > sim->ceiling + 0.10 || sim->peak > c->peak_cap_db + 1.0e-6;
  double prior_sum = 0.0; /* np.mean of four terms: a plain left-to-right sum */
  for (int k = 0; k < CSM_CONTROLS; ++k) {
    const double span = csm_bounds[k][1] - csm_bounds[k][0];
    const double d = (e->values[k] - s->incumbent[k]) / span;
    prior_sum += d * d;
  }
  const double terms[8] = {
      csm_huber((output_lufs - c->target_lufs) / 2.0),
      csm_huber((sim->median - c->target_median_db) / 1.0),
      csm_huber((sim->p95 - c->target_p95_db) / 1.0),
      csm_huber(fmax(0.0, 1.0 - sim->pre_limiter_headroom) / 1.0),
      csm_huber(sim->pumping / 1.0),
      csm_huber(fmax(0.0, sim->silence_gain - 0.25) / 1.0),
      csm_huber(fmax(0.0, 0.20 - sim->active_ratio) / 0.20),
      prior_sum / 4.0,
  };
  static const double weights[8] = {1.00, 0.35, 0.90, 0.45, 0.30, 1.50, 0.25, 0.08}; /* :715-724, in the order of `terms` */
  double score = 0.0;
  for (int i = 0; i < 8; ++i) score += weights[i] * terms[i];
  e->score = hard_rejected ? INFINITY : score;
}

static inline int csm_before(const csm_entry *a, const csm_entry *b) { /* (score, key_for(values)) */
  if (a->score != b->score) return a->score < b->score;
  for (int k = 0; k < CSM_CONTROLS; ++k)
    if (a->value_key[k] != b->value_key[k]) return a->value_key[k] < b->value_key[k];
  return 0;
}

/* sorted(feasible, key=(score, key)), :928-931: indices of the finite-score entries, stable */
static inline int csm_feasible(const csm_search *s, int order[CSM_MAX_EVALUATED]) {
  int m = 0;
  for (int i = 0; i < s->n_scored; ++i) {
    if (!isfinite(s->entries[i].score)) continue;
    int j = m++;
    while (j > 0 && csm_before(&s->entries[i], &s->entries[order[j - 1]])) {
      order[j] = order[j - 1];
      --j;
    }
    order[j] = i;
  }
  return m;
}

static inline int csm_threshold_only(const csm_search *s, const csm_entry *e) { /* :976-979 */
  for (int k = 1; k < CSM_CONTROLS; ++k)
    if (!(fabs(e->values[k] - s->incumbent[k]) <= 1.0e-6)) return 0;
  return 1;
}

/* :928-966.  Returns how many new entries wait for a simulation, or -1 when phase 1 left no feasible candidate. */
static inline int csm_phase2(csm_search *s) {
  int order[CSM_MAX_EVALUATED];
  const int m = csm_feasible(s, order);
  if (m == 0) return -1;
  int seeds[2], n_seeds = 1;
  seeds[0] = order[0];
  int multivariable = -1;
  for (int i = 0; i < m && multivariable < 0; ++i) {
    const csm_entry *e = &s->entries[order[i]];
    for (int k = 1; k < CSM_CONTROLS; ++k)
      if (fabs(e->values[k] - s->incumbent[k]) > 1.0e-6) multivariable = order[i];
  }
  if (multivariable >= 0 && memcmp(s->entries[multivariable].value_key, s->entries[seeds[0]].value_key, sizeof(double) * CSM_CONTROLS) != 0)
    seeds[n_seeds++] = multivariable;
  else if (m > 1)
    seeds[n_seeds++] = order[1];
  for (int q = 0; q < n_seeds; ++q) {
    double seed[CSM_CONTROLS];
    memcpy(seed, s->entries[seeds[q]].values, sizeof seed);
    for (int k = 0; k < CSM_CONTROLS; ++k)
      for (int direction = -1; direction <= 1; direction += 2) {
        double candidate[CSM_CONTROLS];
        memcpy(candidate, seed, sizeof candidate);
        candidate[k] += (double)direction * csm_local_steps[k];
        csm_offer(s, candidate);
      }
  }
  return s->n - s->n_scored;
}

/* :968-995, plus the two objectives of :1028-1049 */
static inline void csm_choose(const csm_search *s, csm_choice *out) {
  int order[CSM_MAX_EVALUATED];
  const int m = csm_feasible(s, order);
  memset(out, 0, sizeof *out);
  out->best = out->expanded = out->threshold_only = -1;
  out->threshold_only_objective = INFINITY;
  out->incumbent_objective = INFINITY;
  double incumbent_key[CSM_CONTROLS];
  for (int k = 0; k < CSM_CONTROLS; ++k) incumbent_key[k] = csm_round6(s->incumbent[k]);
  for (int i = 0; i < s->n_scored; ++i) {
    const csm_entry *e = &s->entries[i];
    if (csm_threshold_only(s, e) && e->score < out->threshold_only_objective) out->threshold_only_objective = e->score;
    if (e->key[0] == incumbent_key[0] && e->key[1] == incumbent_key[1] && e->key[2] == incumbent_key[2] && e->key[3] == incumbent_key[3])
      out->incumbent_objective = e->score;
  }
  if (m == 0) return;
  out->feasible = 1;
  out->expanded = order[0];
  for (int i = 0; i < m && out->threshold_only < 0; ++i)
    if (csm_threshold_only(s, &s->entries[order[i]])) out->threshold_only = order[i];
  if (out->threshold_only < 0) {
    out->expanded_selected = 1;
    out->best = out->expanded;
  } else {
    const double threshold_score = s->entries[out->threshold_only].score;
    const double required = fmax(0.001, 0.01 * threshold_score);
    out->expanded_selected = threshold_score - s->entries[out->expanded].score > required;
    out->best = out->expanded_selected ? out->expanded : out->threshold_only;
  }
}

#endif /* AF_COMPRESSOR_SEARCH_MATH_H */
