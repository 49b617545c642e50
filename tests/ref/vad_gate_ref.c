/* vad_gate_ref.c -- CPU restatement (test infrastructure only) of the reference's noise gate WITH a
 * VadAutoGate::without_backend attached, i.e. the branch of process_block_inplace the realtime loop runs in the modes
 * VadAssisted / VadOnly (rust-core/src/dsp/gate.rs:652-741) and the per-block controller behind it
 * (rust-core/src/dsp/vad.rs:714-966).  Types as in the reference: f32 for the block sum of squares (sequential, in sample
 * order), sqrt, log10, the noise floor, the bins, the hold timer and the closed counter; f64 for the detector, the posterior
 * reduction and the gain; vad_smoothed_probability computed in f64 and stored as f32 per sample.
 * Built with -O2 -ffp-contract=off -fno-fast-math (no reassociation, no fused multiply-add). */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define HISTORY_FRAMES 250 /* vad.rs:57-63 */
#define BIN_COUNT 61
#define BIN_MIN_DB (-80.0f)
#define BIN_STEP_DB 1.0f
#define ELIGIBLE_PROB_MAX 0.3f
#define UP_SLEW 0.5f
#define DOWN_SLEW 0.1f

enum { MODE_THRESHOLD_ONLY = 0, MODE_VAD_ASSISTED = 1, MODE_VAD_ONLY = 2 };
enum { ST_CLOSED = 0, ST_OPENING = 1, ST_OPEN = 2, ST_UNCERTAIN = 3, ST_RELEASING = 4 }; /* gate.rs:53-61 */

static float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }
static double clampd(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }
/* dsp/util.rs: time_constant_to_coeff, db_to_linear, linear_to_db */
static double tc_coeff(double ms, double fs) { return exp(-1.0 / ((fmax(ms, 0.001) / 1000.0) * fs)); }
static double db_to_linear(double db) { return pow(10.0, db / 20.0); }
static double linear_to_db(double lin, double min_lin) { return 20.0 * log10(fmax(fabs(lin), min_lin)); }

/* ---- VadAutoGate (vad.rs:575-624), the fields the without_backend path uses */
typedef struct {
  float noise_floor, margin, min_threshold, max_threshold, manual_threshold_db;
  int auto_threshold_enabled, enabled, gate_mode;
  float vad_threshold, hold_time_ms, hold_timer;
  int timer_running, prev_gate_open;
  float closed_counter_samples, debounce_time_ms;
  uint32_t sample_rate;
  float current_probability;
  int external_probability_available;
  float history[HISTORY_FRAMES];
  size_t history_len, history_cursor;
  uint16_t bins[BIN_COUNT];
  /* diagnostics of the restatement (not reference state): the last block's level and decision, and the smallest distance of
   * any block's rms_db to a histogram bin edge (when it was pushed) or to the level threshold in force */
  float last_rms_db, last_threshold_db, min_edge_distance_db;
  int last_raw_open, last_held_open;
} vad_ctl;

/* vad.rs:663-690 */
static void ctl_init(vad_ctl *c, uint32_t sample_rate, float vad_threshold) {
  memset(c, 0, sizeof *c);
  c->noise_floor = -60.0f;
  c->margin = 10.0f;
  c->min_threshold = -80.0f;
  c->max_threshold = -10.0f;
  c->manual_threshold_db = -40.0f;
  c->auto_threshold_enabled = 1;
  c->enabled = 1;
  c->gate_mode = MODE_THRESHOLD_ONLY;
  c->vad_threshold = vad_threshold;
  c->hold_time_ms = 200.0f;
  c->debounce_time_ms = 50.0f;
  c->closed_counter_samples = (float)sample_rate * 0.05f;
  c->sample_rate = sample_rate;
  c->min_edge_distance_db = INFINITY;
  c->last_rms_db = -120.0f;
}

/* vad.rs:1086-1099 */
static float compute_rms_db(const float *x, size_t n) {
  if (n == 0) return -120.0f;
  float sum = 0.0f;
  for (size_t i = 0; i < n; ++i) sum += x[i] * x[i];
  const float rms = sqrtf(sum / (float)n);
  if (rms < 1e-6f) return -120.0f;
  return 20.0f * log10f(rms);
}

/* vad.rs:823-826 */
static size_t noise_floor_bin(float db) {
  const float raw = roundf((db - BIN_MIN_DB) / BIN_STEP_DB);
  return (size_t)clampf(raw, 0.0f, (float)(BIN_COUNT - 1));
}

/* vad.rs:763-780 (saturating u16 arithmetic) */
static void push_noise_floor_sample(vad_ctl *c, float db) {
  const size_t bin = noise_floor_bin(db);
  if (c->history_len < HISTORY_FRAMES) {
    c->history[c->history_len++] = db;
    if (c->bins[bin] < UINT16_MAX) c->bins[bin] += 1;
    return;
  }
  const size_t old_bin = noise_floor_bin(c->history[c->history_cursor]);
  if (c->bins[old_bin] > 0) c->bins[old_bin] -= 1;
  c->history[c->history_cursor] = db;
  if (c->bins[bin] < UINT16_MAX) c->bins[bin] += 1;
  c->history_cursor = (c->history_cursor + 1) % HISTORY_FRAMES;
}

/* vad.rs:786-802; returns 0 for None */
static int noise_floor_percentile(const vad_ctl *c, float percentile, float *out) {
  if (c->history_len == 0) return 0;
  size_t target = (size_t)floorf((float)c->history_len * clampf(percentile, 0.0f, 1.0f));
  if (target > c->history_len - 1) target = c->history_len - 1;
  size_t cumulative = 0;
  for (size_t bin = 0; bin < BIN_COUNT; ++bin) {
    cumulative += c->bins[bin];
    if (cumulative > target) {
      *out = BIN_MIN_DB + (float)bin * BIN_STEP_DB;
      return 1;
    }
  }
  *out = c->noise_floor;
  return 1;
}

/* vad.rs:805-821 */
static float noise_floor_reliability(const vad_ctl *c) {
  if (c->history_len == 0) return 0.0f;
  const float maturity = clampf((float)c->history_len / (float)HISTORY_FRAMES, 0.0f, 1.0f);
  float p20, p80;
  if (!noise_floor_percentile(c, 0.20f, &p20)) return 0.0f;
  if (!noise_floor_percentile(c, 0.80f, &p80)) return 0.0f;
  const float spread = fmaxf(p80 - p20, 0.0f);
  const float t = clampf((spread - 3.0f) / 7.0f, 0.0f, 1.0f);
  const float stationarity = 1.0f - t * t * (3.0f - 2.0f * t);
  return clampf(maturity * stationarity, 0.0f, 1.0f);
}

static void note_edge(vad_ctl *c, float d) {
  d = fabsf(d);
  if (d < c->min_edge_distance_db) c->min_edge_distance_db = d;
}

/* vad.rs:728-761 */
static void update_noise_floor_estimate(vad_ctl *c, float current_rms, float prob) {
  if (!c->auto_threshold_enabled || prob >= ELIGIBLE_PROB_MAX) return;
  if (current_rms <= -100.0f) return;
  {
    const float pos = (current_rms - BIN_MIN_DB) / BIN_STEP_DB;  /* bin edges sit at k + 0.5 inside the clamp */
    if (pos > -1.0f && pos < (float)BIN_COUNT) note_edge(c, (pos - floorf(pos)) - 0.5f);
  }
  push_noise_floor_sample(c, current_rms);
  float candidate;
  if (!noise_floor_percentile(c, 0.20f, &candidate)) return;
  const float delta = candidate - c->noise_floor;
  if (delta > 0.0f)
    c->noise_floor += fminf(delta, UP_SLEW);
  else
    c->noise_floor += fmaxf(delta, -DOWN_SLEW);
  c->noise_floor = clampf(c->noise_floor, -80.0f, -20.0f);
}

/* vad.rs:912-923 */
static int level_above_threshold(vad_ctl *c, float rms_db) {
  const float threshold = c->auto_threshold_enabled ? clampf(c->noise_floor + c->margin, c->min_threshold, c->max_threshold)
                                                    : clampf(c->manual_threshold_db, c->min_threshold, c->max_threshold);
  c->last_threshold_db = threshold;
  note_edge(c, rms_db - threshold);
  return rms_db >= threshold;
}

/* vad.rs:925-966 */
static int apply_hold_time(vad_ctl *c, int gate_open, size_t num_samples) {
  const float debounce_samples = c->debounce_time_ms / 1000.0f * (float)c->sample_rate;
  const int rising_edge = gate_open && !c->prev_gate_open;
  const int debounce_ready = c->closed_counter_samples >= debounce_samples;
  const int debounced = (rising_edge && !debounce_ready) ? 0 : gate_open;
  if (debounced) {
    c->hold_timer = c->hold_time_ms / 1000.0f * (float)c->sample_rate;
    c->timer_running = 1;
    c->closed_counter_samples = 0.0f;
  } else {
    c->closed_counter_samples += (float)num_samples;
  }
  if (c->timer_running) {
    c->hold_timer -= (float)num_samples;
    if (c->hold_timer <= 0.0f) {
      c->hold_timer = 0.0f;
      c->timer_running = 0;
    }
  }
  c->prev_gate_open = debounced;
  return debounced || c->timer_running;
}

/* vad.rs:828-910 */
static int process_with_probability(vad_ctl *c, const float *x, size_t n, float prob) {
  c->current_probability = prob;
  const int speech = prob > c->vad_threshold;
  const float rms_db = compute_rms_db(x, n);
  c->last_rms_db = rms_db;
  update_noise_floor_estimate(c, rms_db, prob);
  const int level = level_above_threshold(c, rms_db);
  int gate_open;
  switch (c->gate_mode) {
    case MODE_VAD_ASSISTED: gate_open = level || speech; break;
    case MODE_VAD_ONLY: gate_open = speech; break;
    default: gate_open = level; break;
  }
  c->last_raw_open = gate_open;
  c->last_held_open = apply_hold_time(c, gate_open, n);
  return c->last_held_open;
}

/* vad.rs:1017-1031 */
static void ctl_reset(vad_ctl *c) {
  c->noise_floor = -60.0f;
  c->hold_timer = 0.0f;
  c->timer_running = 0;
  c->prev_gate_open = 0;
  c->closed_counter_samples = c->debounce_time_ms / 1000.0f * (float)c->sample_rate;
  c->current_probability = 0.0f;
  memset(c->history, 0, sizeof c->history);
  c->history_len = 0;
  c->history_cursor = 0;
  memset(c->bins, 0, sizeof c->bins);
}

/* ---- NoiseGate (gate.rs:78-156) */
typedef struct {
  double threshold_db, attack_coeff, release_coeff, rms_envelope_sq, rms_coeff, detector_level_db;
  size_t hold_remaining_samples;
  double current_gain, sample_rate;
  int is_open, enabled;
  int effective_gate_open, has_effective_gate_state;
  size_t chatter_window_remaining_samples;
  uint32_t chatter_transition_count;
  size_t chatter_cooldown_samples;
  uint64_t chatter_event_count;
  int gate_mode;
  int has_vad; /* Option<VadAutoGate> */
  vad_ctl vad;
  float vad_external_probability;
  int vad_external_available;
  float fused_gate_score;
  int fused_gate_open, gate_state;
  float previous_vad_probability, vad_smoothed_probability;
  double vad_probability_smoothing_coeff;
  size_t auto_relax_remaining_samples;
  int visited_states; /* diagnostics of the restatement: bit k set once gate_state == k was held after a sample */
  uint32_t vad_opened_below_level; /* samples the fused gate ran not force-closed while the detector's is_open was false */
} vad_gate;

/* gate.rs:158-225 */
static void gate_init(vad_gate *g, double threshold_db, double attack_ms, double release_ms, double fs) {
  memset(g, 0, sizeof *g);
  g->threshold_db = threshold_db;
  g->attack_coeff = tc_coeff(attack_ms, fs);
  g->release_coeff = tc_coeff(release_ms, fs);
  g->rms_coeff = tc_coeff(8.0, fs);
  g->detector_level_db = -120.0;
  g->sample_rate = fs;
  g->enabled = 1;
  g->gate_mode = MODE_THRESHOLD_ONLY;
  g->gate_state = ST_CLOSED;
  g->vad_probability_smoothing_coeff = tc_coeff(35.0, fs);
}

static int auto_relax_active(const vad_gate *g) { return g->auto_relax_remaining_samples > 0; }
static double expander_range_db(const vad_gate *g) { return auto_relax_active(g) ? 24.0 : 36.0; } /* gate.rs:287-295 */

/* gate.rs:265-285 */
static void update_detector(vad_gate *g, double input) {
  g->rms_envelope_sq = g->rms_coeff * g->rms_envelope_sq + (1.0 - g->rms_coeff) * input * input;
  g->detector_level_db = linear_to_db(sqrt(g->rms_envelope_sq), 1e-10);
  if (g->detector_level_db >= g->threshold_db) {
    g->is_open = 1;
    g->hold_remaining_samples = (size_t)round(g->sample_rate * 50.0 / 1000.0);
  } else if (g->hold_remaining_samples > 0) {
    g->hold_remaining_samples -= 1;
    g->is_open = 1;
  } else if (g->detector_level_db <= g->threshold_db - 4.0) {
    g->is_open = 0;
  }
}

/* gate.rs:297-306 */
static double detector_gain_reduction_db(const vad_gate *g) {
  if (g->is_open) return 0.0;
  return clampd((g->threshold_db - g->detector_level_db) * (1.0 - 1.0 / 4.0), 0.0, expander_range_db(g));
}

/* gate.rs:307-313 */
static float level_open_score(const vad_gate *g) {
  const double closed_db = g->threshold_db - 4.0;
  const double score = (g->detector_level_db - closed_db) / (g->threshold_db - closed_db);
  return (float)clampd(score, 0.0, 1.0);
}

/* gate.rs:315-366 */
static int update_fused_gate_score(vad_gate *g, int mode, float vad_probability, int vad_available, int vad_held_open) {
  const float level_score = level_open_score(g);
  const float vad_score = clampf(vad_probability, 0.0f, 1.0f);
  const float recent_score = (g->fused_gate_open || g->current_gain > 0.35) ? 1.0f : 0.0f;
  switch (mode) {
    case MODE_VAD_ASSISTED:
      if (vad_available) {
        const float blended = clampf(0.55f * level_score + 0.45f * vad_score + 0.10f * recent_score, 0.0f, 1.0f);
        g->fused_gate_score = fmaxf(fmaxf(level_score, vad_score), blended);
      } else {
        g->fused_gate_score = 0.85f * level_score + 0.15f * recent_score;
      }
      break;
    case MODE_VAD_ONLY:
      if (vad_available)
        g->fused_gate_score = vad_held_open ? fmaxf(vad_score, 0.55f) : vad_score;
      else
        g->fused_gate_score = vad_held_open ? 0.55f : 0.0f;
      break;
    default: g->fused_gate_score = level_score; break;
  }
  if (g->fused_gate_score >= 0.55f)
    g->fused_gate_open = 1;
  else if (g->fused_gate_score <= 0.35f)
    g->fused_gate_open = 0;
  return g->fused_gate_open;
}

/* gate.rs:374-483 */
static int update_probabilistic_gate_state(vad_gate *g, int mode, float vad_probability, int vad_available, int vad_held_open,
                                           float vad_threshold, float probability_delta) {
  const float level_score = level_open_score(g);
  const int auto_relax = auto_relax_active(g);
  const float close_margin = auto_relax ? 0.20f : 0.12f;
  const float open_threshold = clampf(vad_threshold, 0.05f, 0.95f);
  const float close_threshold = clampf(open_threshold - close_margin, 0.02f, open_threshold);
  const int vad_open = vad_available && (vad_probability >= open_threshold ||
                                         (probability_delta >= 0.08f && vad_probability >= close_threshold));
  const int vad_uncertain = vad_available && vad_probability >= close_threshold;
  const int level_open = g->is_open || level_score >= 0.55f;
  const int level_uncertain = level_score >= 0.22f || g->current_gain > 0.12;
  const int carry = !vad_available || vad_uncertain || g->current_gain > 0.20;
  const int level_speech_candidate = level_open && carry;
  const int fused_speech_candidate = g->fused_gate_open && carry;
  const int vad_hold_candidate = vad_held_open && carry;
  int strong_open, sustain;
  switch (mode) {
    case MODE_VAD_ASSISTED:
      strong_open = level_speech_candidate || fused_speech_candidate || vad_hold_candidate || vad_open;
      sustain = strong_open || vad_uncertain || level_uncertain || (auto_relax && level_score > 0.08f);
      break;
    case MODE_VAD_ONLY:
      strong_open = vad_held_open || vad_open;
      sustain = strong_open || vad_uncertain || (auto_relax && g->current_gain > 0.12);
      break;
    default:
      strong_open = level_open;
      sustain = level_open;
      break;
  }
  const int releasing_sustain = sustain || (g->current_gain > 0.20 && (vad_uncertain || auto_relax));
  switch (g->gate_state) {
    case ST_CLOSED: g->gate_state = strong_open ? ST_OPENING : ST_CLOSED; break;
    case ST_OPENING: g->gate_state = strong_open ? ST_OPEN : (sustain ? ST_UNCERTAIN : ST_CLOSED); break;
    case ST_OPEN:
      g->gate_state = strong_open ? ST_OPEN : (sustain ? ST_UNCERTAIN : (releasing_sustain ? ST_RELEASING : ST_CLOSED));
      break;
    default: /* Uncertain and Releasing share their transitions */
      g->gate_state = strong_open ? ST_OPENING : (sustain ? ST_UNCERTAIN : (releasing_sustain ? ST_RELEASING : ST_CLOSED));
      break;
  }
  return g->gate_state != ST_CLOSED;
}

/* gate.rs:485-496 */
static double probability_speech_confidence(float probability, float vad_threshold) {
  const float open_threshold = clampf(vad_threshold, 0.05f, 0.95f);
  const float close_threshold = clampf(open_threshold - 0.20f, 0.02f, fmaxf(open_threshold - 0.02f, 0.02f));
  const float span = fmaxf(open_threshold - close_threshold, 1.0e-3f);
  const double normalized = (double)clampf((probability - close_threshold) / span, 0.0f, 1.0f);
  return normalized * normalized * (3.0 - 2.0 * normalized);
}

/* gate.rs:498-527 */
static double continuous_vad_gain_reduction_db(const vad_gate *g, int mode, float probability, int vad_available,
                                               int vad_held_open, float vad_threshold) {
  if (!vad_available) return 0.0;
  double closure = 1.0 - probability_speech_confidence(probability, vad_threshold);
  if (vad_held_open && probability >= (vad_threshold - 0.20f)) closure = fmin(closure, 0.80);
  const double scale = mode == MODE_VAD_ASSISTED ? 0.30 : (mode == MODE_VAD_ONLY ? 0.45 : 0.0);
  return expander_range_db(g) * closure * scale;
}

/* gate.rs:529-553 */
static double compute_vad_target_gr_db(const vad_gate *g, int mode, float probability, int vad_available, int vad_held_open,
                                       float vad_threshold, int force_close) {
  if (force_close) return expander_range_db(g);
  const double level_reduction = detector_gain_reduction_db(g);
  const double posterior = continuous_vad_gain_reduction_db(g, mode, probability, vad_available, vad_held_open, vad_threshold);
  return fmax(level_reduction, posterior);
}

/* gate.rs:573-588 */
static void advance_chatter_timers(vad_gate *g) {
  if (g->auto_relax_remaining_samples > 0) g->auto_relax_remaining_samples -= 1;
  if (g->chatter_window_remaining_samples > 0) {
    g->chatter_window_remaining_samples -= 1;
    if (g->chatter_window_remaining_samples == 0) g->chatter_transition_count = 0;
  }
  if (g->chatter_cooldown_samples > 0) g->chatter_cooldown_samples -= 1;
}

/* gate.rs:590-623 */
static void track_gate_transition(vad_gate *g, int effective_open) {
  if (!g->has_effective_gate_state) {
    g->effective_gate_open = effective_open;
    g->has_effective_gate_state = 1;
    advance_chatter_timers(g);
    return;
  }
  if (effective_open != g->effective_gate_open) {
    g->effective_gate_open = effective_open;
    if (g->chatter_window_remaining_samples == 0) {
      g->chatter_window_remaining_samples = (size_t)round(g->sample_rate * 500.0 / 1000.0);
      g->chatter_transition_count = 1;
    } else if (g->chatter_transition_count < UINT32_MAX) {
      g->chatter_transition_count += 1;
    }
    if (g->chatter_transition_count >= 4 && g->chatter_cooldown_samples == 0) {
      g->chatter_event_count += 1;
      g->chatter_cooldown_samples = (size_t)round(g->sample_rate * 1000.0 / 1000.0);
      if (g->gate_mode != MODE_THRESHOLD_ONLY) g->auto_relax_remaining_samples = (size_t)round(g->sample_rate * 700.0 / 1000.0);
      g->chatter_window_remaining_samples = 0;
      g->chatter_transition_count = 0;
    }
  }
  advance_chatter_timers(g);
}

/* gate.rs:625-635 */
static float apply_gain(vad_gate *g, double input, double target_gr_db) {
  const double target_gain = db_to_linear(-target_gr_db);
  const double coeff = target_gain > g->current_gain ? g->attack_coeff : g->release_coeff;
  g->current_gain = coeff * g->current_gain + (1.0 - coeff) * target_gain;
  return (float)(input * g->current_gain);
}

/* gate.rs:637-649 */
static float process_sample(vad_gate *g, float input) {
  if (!g->enabled) return input;
  const double x = (double)input;
  update_detector(g, x);
  const double gr = detector_gain_reduction_db(g); /* compute_target_gr_db(false), gate.rs:555-561 */
  track_gate_transition(g, g->is_open);
  return apply_gain(g, x, gr);
}

/* gate.rs:651-756 */
static void process_block_inplace(vad_gate *g, float *buf, size_t n) {
  if (!g->enabled) return;
  if (g->gate_mode != MODE_THRESHOLD_ONLY && g->has_vad && g->vad.enabled) {
    vad_ctl *c = &g->vad;
    /* process_with_external_probability, vad.rs:714-726 */
    c->external_probability_available = g->vad_external_available;
    const float probability = clampf(g->vad_external_available ? g->vad_external_probability : 0.0f, 0.0f, 1.0f);
    const int vad_gate_open = process_with_probability(c, buf, n, probability);
    const float vad_threshold = c->vad_threshold;
    const int available = g->vad_external_available;
    const float probability_delta = probability - g->previous_vad_probability;
    const double k = g->vad_probability_smoothing_coeff;
    for (size_t i = 0; i < n; ++i) {
      const double x = (double)buf[i];
      g->vad_smoothed_probability = (float)clampd(k * (double)g->vad_smoothed_probability + (1.0 - k) * (double)probability, 0.0, 1.0);
      update_detector(g, x);
      update_fused_gate_score(g, g->gate_mode, probability, available, vad_gate_open);
      const int probabilistic_open =
          update_probabilistic_gate_state(g, g->gate_mode, probability, available, vad_gate_open, vad_threshold, probability_delta);
      const int force_close = g->gate_mode != MODE_THRESHOLD_ONLY && !probabilistic_open;
      const double gr = compute_vad_target_gr_db(g, g->gate_mode, g->vad_smoothed_probability, available, vad_gate_open,
                                                 vad_threshold, force_close);
      const int effective_open = !force_close && probabilistic_open;
      track_gate_transition(g, effective_open);
      buf[i] = apply_gain(g, x, gr);
      g->visited_states |= 1 << g->gate_state;
      if (effective_open && !g->is_open) g->vad_opened_below_level += 1;
    }
    g->previous_vad_probability = probability;
    return;
  }
  for (size_t i = 0; i < n; ++i) buf[i] = process_sample(g, buf[i]);
}

/* gate.rs:758-784 (the attached controller is NOT reset here; vgr_ctl_reset is VadAutoGate::reset) */
static void gate_reset(vad_gate *g) {
  g->current_gain = 0.0;
  g->rms_envelope_sq = 0.0;
  g->detector_level_db = -120.0;
  g->hold_remaining_samples = 0;
  g->is_open = 0;
  g->effective_gate_open = 0;
  g->has_effective_gate_state = 0;
  g->chatter_window_remaining_samples = 0;
  g->chatter_transition_count = 0;
  g->chatter_cooldown_samples = 0;
  g->chatter_event_count = 0;
  g->vad_external_probability = 0.0f;
  g->vad_external_available = 0;
  g->fused_gate_score = 0.0f;
  g->fused_gate_open = 0;
  g->gate_state = ST_CLOSED;
  g->previous_vad_probability = 0.0f;
  g->vad_smoothed_probability = 0.0f;
  g->auto_relax_remaining_samples = 0;
}

/* ================================================================= the ctypes surface */
typedef struct {
  float current_gain, fused_gate_score, vad_smoothed_probability, noise_floor, noise_floor_reliability;
  float last_rms_db, last_threshold_db, min_edge_distance_db, hold_timer, closed_counter_samples;
  int32_t is_open, gate_state, auto_relax_active, fused_gate_open, held_open, raw_open, history_len, visited_states;
  uint64_t chatter_event_count;
  uint32_t vad_opened_below_level;
  int32_t floor_bin; /* noise_floor_bin(noise_floor) */
} vgr_report;

void *vgr_new(double threshold_db, double attack_ms, double release_ms, double fs) {
  vad_gate *g = malloc(sizeof *g);
  if (g) gate_init(g, threshold_db, attack_ms, release_ms, fs);
  return g;
}
void vgr_free(void *p) { free(p); }
/* set_vad_auto_gate, gate.rs:829-836: Some(VadAutoGate::without_backend(fs, vad_threshold)) or None */
void vgr_attach(void *p, int on, float vad_threshold) {
  vad_gate *g = p;
  g->has_vad = on != 0;
  if (on) {
    ctl_init(&g->vad, (uint32_t)g->sample_rate, vad_threshold);
    g->vad.gate_mode = MODE_THRESHOLD_ONLY;
    g->vad.manual_threshold_db = clampf((float)g->threshold_db, g->vad.min_threshold, g->vad.max_threshold); /* vad.rs:996-999 */
  }
}
/* gate.rs:810-821, vad.rs:1033-1037 */
void vgr_set_mode(void *p, int mode) {
  vad_gate *g = p;
  g->gate_mode = mode;
  if (mode == MODE_THRESHOLD_ONLY) {
    g->gate_state = ST_CLOSED;
    g->auto_relax_remaining_samples = 0;
  }
  if (g->has_vad) g->vad.gate_mode = mode;
}
/* gate.rs:227-233 */
void vgr_set_threshold(void *p, double threshold_db) {
  vad_gate *g = p;
  g->threshold_db = threshold_db;
  if (g->has_vad) g->vad.manual_threshold_db = clampf((float)threshold_db, g->vad.min_threshold, g->vad.max_threshold);
}
void vgr_set_attack_time(void *p, double ms) { vad_gate *g = p; g->attack_coeff = tc_coeff(ms, g->sample_rate); }
void vgr_set_release_time(void *p, double ms) { vad_gate *g = p; g->release_coeff = tc_coeff(ms, g->sample_rate); }
void vgr_set_enabled(void *p, int on) { ((vad_gate *)p)->enabled = on != 0; }
/* gate.rs:838-843 */
void vgr_set_external_vad_probability(void *p, float probability, int available) {
  vad_gate *g = p;
  g->vad_external_probability = clampf(probability, 0.0f, 1.0f);
  g->vad_external_available = available != 0;
}
/* gate.rs:866-915 over vad.rs:984, 1002-1010, 1043-1056: no-ops without a controller */
void vgr_set_vad_threshold(void *p, float v) { vad_gate *g = p; if (g->has_vad) g->vad.vad_threshold = clampf(v, 0.0f, 1.0f); }
void vgr_set_hold_time(void *p, float ms) { vad_gate *g = p; if (g->has_vad) g->vad.hold_time_ms = clampf(ms, 0.0f, 500.0f); }
void vgr_set_margin(void *p, float db) { vad_gate *g = p; if (g->has_vad) g->vad.margin = clampf(db, 0.0f, 20.0f); }
void vgr_set_auto_threshold(void *p, int on) {
  vad_gate *g = p;
  if (!g->has_vad) return;
  g->vad.auto_threshold_enabled = on != 0;
  if (on && g->vad.noise_floor <= -100.0f) g->vad.noise_floor = -60.0f;
}
void vgr_process_block(void *p, float *buf, size_t n) { process_block_inplace(p, buf, n); }
float vgr_process_sample(void *p, float x) { return process_sample(p, x); }
void vgr_reset(void *p) { gate_reset(p); }
void vgr_ctl_reset(void *p) { vad_gate *g = p; if (g->has_vad) ctl_reset(&g->vad); }
void vgr_set_current_gain(void *p, double gain) { ((vad_gate *)p)->current_gain = gain; }
double vgr_current_gain_f64(void *p) { return ((vad_gate *)p)->current_gain; }
float vgr_apply_gain(void *p, double input, double target_gr_db) { return apply_gain(p, input, target_gr_db); }
double vgr_continuous_vad_gain_reduction_db(void *p, int mode, float probability, int available, int held, float vad_threshold) {
  return continuous_vad_gain_reduction_db(p, mode, probability, available, held, vad_threshold);
}
/* is_vad_available, gate.rs:845-852 over vad.rs:968-974 */
int vgr_is_vad_available(void *p) { vad_gate *g = p; return g->has_vad ? g->vad.external_probability_available : 0; }
void vgr_report_state(void *p, vgr_report *r) {
  vad_gate *g = p;
  memset(r, 0, sizeof *r);
  r->current_gain = (float)g->current_gain;
  r->fused_gate_score = g->fused_gate_score;
  r->vad_smoothed_probability = g->vad_smoothed_probability;
  r->noise_floor = g->has_vad ? g->vad.noise_floor : -60.0f;                          /* gate.rs:935-942 */
  r->noise_floor_reliability = g->has_vad ? noise_floor_reliability(&g->vad) : 0.0f;  /* gate.rs:944-951 */
  r->is_open = g->is_open;
  r->gate_state = g->gate_state;
  r->auto_relax_active = auto_relax_active(g);
  r->fused_gate_open = g->fused_gate_open;
  r->chatter_event_count = g->chatter_event_count;
  r->visited_states = g->visited_states;
  r->vad_opened_below_level = g->vad_opened_below_level;
  r->min_edge_distance_db = INFINITY;
  if (g->has_vad) {
    r->last_rms_db = g->vad.last_rms_db;
    r->last_threshold_db = g->vad.last_threshold_db;
    r->min_edge_distance_db = g->vad.min_edge_distance_db;
    r->hold_timer = g->vad.hold_timer;
    r->closed_counter_samples = g->vad.closed_counter_samples;
    r->held_open = g->vad.last_held_open;
    r->raw_open = g->vad.last_raw_open;
    r->history_len = (int32_t)g->vad.history_len;
    r->floor_bin = (int32_t)noise_floor_bin(g->vad.noise_floor);
  }
}
/* the controller on its own (vad/tests.rs drives it directly) */
int vgr_ctl_process_with_probability(void *p, const float *x, size_t n, float prob) {
  vad_gate *g = p;
  return process_with_probability(&g->vad, x, n, prob);
}
void vgr_ctl_push_noise_floor_sample(void *p, float db) { push_noise_floor_sample(&((vad_gate *)p)->vad, db); }
float vgr_compute_rms_db(const float *x, size_t n) { return compute_rms_db(x, n); }
double vgr_db_to_linear(double db) { return db_to_linear(db); }
