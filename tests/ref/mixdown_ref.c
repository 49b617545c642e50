/* CPU restatement of the reference's input mixdown, operation for operation (test infrastructure only).
 *
 * Restates rust-core/src/audio/input.rs:84-135 (PhaseSafeMonoState: push, lagrange_sample), :383-736
 * (strongest_channel_index, stereo_correlation, delayed_correlation, best_phase_alignment, mix_phase_safe_stereo,
 * mix_interleaved_to_mono_with_mode_and_state) and the input callback's wrapper :789-842 (one-channel copy; otherwise
 * chunks of at most 8192 frames, one decision per chunk, the per-stream diagnostics).
 *
 * f32 input only: the reference takes i16 / u16 device formats through a cpal sample conversion that is not part of its
 * tree, so only the f32 path (an identity conversion) can be restated.
 *
 * Every quantity is an IEEE f32 add / mul / div / sqrt in the reference's order: build with -ffp-contract=off and
 * without fast-math (tests/mixdown_oracle.py does).  The branch counters exist for tests/test_mixdown_stimulus.py. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define MAX_DELAY 8                     /* PHASE_SAFE_MAX_DELAY_SAMPLES, input.rs:25 */
#define MIN_CORRELATION 0.35f           /* :26 */
#define MIN_IMPROVEMENT 0.04f           /* :27 */
#define HISTORY 16                      /* :28 */
#define LATENCY 2.0f                    /* :29 */
#define WARNING_CORRELATION (-0.75f)    /* :24 */
#define SCRATCH_CAPACITY 8192           /* :778 */
#define F32_EPSILON 1.1920929e-07f
#define FRAC_1_SQRT_2 0.70710678118654752440f

enum { MODE_AVERAGE = 0, MODE_LEFT = 1, MODE_RIGHT = 2, MODE_MAX_RMS = 3, MODE_PHASE_SAFE_MONO = 4 };
enum { STRATEGY_NONE = 0, STRATEGY_POLARITY_FLIP = 1, STRATEGY_FRACTIONAL_DELAY = 2, STRATEGY_MAX_RMS_FALLBACK = 3 };

enum {
  CNT_STRATEGY_NONE = 0,      /* chunks mixed by each strategy (phase-safe stereo only) */
  CNT_STRATEGY_FLIP,
  CNT_STRATEGY_FRACTIONAL,
  CNT_STRATEGY_FALLBACK,
  CNT_WARM_UP,                /* frames emitted by the warm-up branch (filled <= required_history) */
  CNT_LAGRANGE_CLAMP,         /* lagrange_sample calls whose delay lay on or beyond a bound of the clamp (the mix passes
                                 2 + |delay| with |delay| <= 8.5: never beyond; the undelayed side sits on the lower bound) */
  CNT_BEST_DELAY_EDGE,        /* detections with best_delay = +-8 (no parabola) */
  CNT_PARABOLA_FLAT,          /* detections whose parabola denominator was <= 1e-6 in magnitude */
  CNT_PARABOLA_MISSING,       /* detections with a neighbour correlation of None */
  CNT_DELAYED_NONE_SHORT,     /* delayed_correlation: None for fewer than 3 overlapping frames */
  CNT_DELAYED_NONE_DENOM,     /* delayed_correlation: None for denom <= EPSILON */
  CNT_STEREO_NONE,            /* stereo_correlation: None */
  CNT_HYSTERESIS_REUSED,      /* nothing detected, correlation < -0.75, a stored candidate reused */
  CNT_HYSTERESIS_CLEARED,     /* nothing detected, correlation >= -0.75, a stored candidate cleared */
  CNT_TIE,                    /* a later lag equalled the running best and lost to the strict > */
  CNT_COUNT
};

typedef struct { int valid; int strategy; float delay_samples, polarity, correlation; } candidate_t;
typedef struct { int strategy; float estimated_delay_samples; int polarity_flipped; } mix_diag_t;
typedef struct { int some; float value; } opt_f32;

typedef struct {
  float left_history[HISTORY], right_history[HISTORY];
  size_t filled;
  candidate_t last_candidate;
} phase_state_t;

typedef struct {
  int n_channels, mode;
  phase_state_t state;
  /* InputStreamOptions' atomics, :181-186 */
  float stereo_correlation;        /* NaN until a first Some */
  uint64_t phase_warning_count;
  int strategy;
  float estimated_delay;
  int polarity_flipped;
  uint64_t counters[CNT_COUNT];
  float scratch[SCRATCH_CAPACITY];
} mixdown_t;

static _Thread_local uint64_t *t_cnt;  /* the counters of the stream this thread is running */
#define COUNT(k) do { if (t_cnt) t_cnt[k]++; } while (0)

static float clampf(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }  /* f32::clamp */

/* :107-117 */
static void state_push(phase_state_t *s, float left, float right) {
  memmove(s->left_history + 1, s->left_history, sizeof(float) * (HISTORY - 1));
  memmove(s->right_history + 1, s->right_history, sizeof(float) * (HISTORY - 1));
  s->left_history[0] = left;
  s->right_history[0] = right;
  s->filled = s->filled + 1 < HISTORY ? s->filled + 1 : HISTORY;
}

/* :121-134 */
static float lagrange_sample(const float *history, float delay) {
  if (delay <= 2.0f || delay >= (float)(HISTORY - 3)) COUNT(CNT_LAGRANGE_CLAMP);
  delay = clampf(delay, 2.0f, (float)(HISTORY - 3));
  const size_t upper_delay = (size_t)ceilf(delay);
  const float t = (float)upper_delay - delay;
  const float x0 = history[upper_delay + 1], x1 = history[upper_delay], x2 = history[upper_delay - 1], x3 = history[upper_delay - 2];
  const float l0 = -t * (t - 1.0f) * (t - 2.0f) / 6.0f;
  const float l1 = (t + 1.0f) * (t - 1.0f) * (t - 2.0f) / 2.0f;
  const float l2 = -(t + 1.0f) * t * (t - 2.0f) / 2.0f;
  const float l3 = (t + 1.0f) * t * (t - 1.0f) / 6.0f;
  return x0 * l0 + x1 * l1 + x2 * l2 + x3 * l3;
}

/* :383-407 */
static size_t strongest_channel_index(const float *x, size_t num_channels, size_t frame_count) {
  size_t best_channel = 0;
  float best_energy = -INFINITY;
  for (size_t channel = 0; channel < num_channels; ++channel) {
    float energy = 0.0f;
    for (size_t frame = 0; frame < frame_count; ++frame) {
      const float sample = x[frame * num_channels + channel];
      energy += sample * sample;
    }
    if (energy > best_energy) {
      best_energy = energy;
      best_channel = channel;
    }
  }
  return best_channel;
}

static opt_f32 correlation_of(float sum_lr, float sum_l2, float sum_r2, int counter) {
  opt_f32 r = {0, 0.0f};
  const float denom = sqrtf(sum_l2 * sum_r2);
  if (denom <= F32_EPSILON) {
    COUNT(counter);
    return r;
  }
  r.some = 1;
  r.value = clampf(sum_lr / denom, -1.0f, 1.0f);
  return r;
}

/* :409-435 */
static opt_f32 stereo_correlation(const float *x, size_t frame_count) {
  if (frame_count == 0) {
    opt_f32 r = {0, 0.0f};
    COUNT(CNT_STEREO_NONE);
    return r;
  }
  float sum_lr = 0.0f, sum_l2 = 0.0f, sum_r2 = 0.0f;
  for (size_t f = 0; f < frame_count; ++f) {
    const float left = x[2 * f], right = x[2 * f + 1];
    sum_lr += left * right;
    sum_l2 += left * left;
    sum_r2 += right * right;
  }
  return correlation_of(sum_lr, sum_l2, sum_r2, CNT_STEREO_NONE);
}

/* :437-475 */
static opt_f32 delayed_correlation(const float *x, size_t frame_count, int delay, float polarity) {
  const size_t start = delay < 0 ? (size_t)(-delay) : 0;
  size_t end = frame_count;
  if (delay > 0) end = frame_count > (size_t)delay ? frame_count - (size_t)delay : 0;
  if ((end > start ? end - start : 0) < 3) {
    opt_f32 r = {0, 0.0f};
    COUNT(CNT_DELAYED_NONE_SHORT);
    return r;
  }
  float sum_lr = 0.0f, sum_l2 = 0.0f, sum_r2 = 0.0f;
  for (size_t left_idx = start; left_idx < end; ++left_idx) {
    const size_t right_idx = (size_t)((int)left_idx + delay);
    const float left = x[left_idx * 2];
    const float right = x[right_idx * 2 + 1] * polarity;
    sum_lr += left * right;
    sum_l2 += left * left;
    sum_r2 += right * right;
  }
  return correlation_of(sum_lr, sum_l2, sum_r2, CNT_DELAYED_NONE_DENOM);
}

/* :477-537 */
static candidate_t best_phase_alignment(const float *x, size_t frame_count, float current_correlation) {
  candidate_t none = {0, STRATEGY_NONE, 0.0f, 0.0f, 0.0f};
  int best_delay = 0;
  float best_polarity = 1.0f, best_corr = -INFINITY;
  static const float polarities[2] = {1.0f, -1.0f};
  for (int p = 0; p < 2; ++p) {
    for (int delay = -MAX_DELAY; delay <= MAX_DELAY; ++delay) {
      const opt_f32 corr = delayed_correlation(x, frame_count, delay, polarities[p]);
      if (corr.some) {
        if (corr.value > best_corr) {
          best_corr = corr.value;
          best_delay = delay;
          best_polarity = polarities[p];
        } else if (corr.value == best_corr) {
          COUNT(CNT_TIE);
        }
      }
    }
  }
  if (best_corr < MIN_CORRELATION || best_corr - current_correlation < MIN_IMPROVEMENT) return none;

  float refined_delay = (float)best_delay;
  if (best_delay > -MAX_DELAY && best_delay < MAX_DELAY) {
    const opt_f32 prev = delayed_correlation(x, frame_count, best_delay - 1, best_polarity);
    const opt_f32 center = delayed_correlation(x, frame_count, best_delay, best_polarity);
    const opt_f32 next = delayed_correlation(x, frame_count, best_delay + 1, best_polarity);
    if (prev.some && center.some && next.some) {
      const float denom = prev.value - 2.0f * center.value + next.value;
      if (fabsf(denom) > 1e-6f) {
        const float offset = clampf(0.5f * (prev.value - next.value) / denom, -0.5f, 0.5f);
        refined_delay += offset;
      } else {
        COUNT(CNT_PARABOLA_FLAT);
      }
    } else {
      COUNT(CNT_PARABOLA_MISSING);
    }
  } else {
    COUNT(CNT_BEST_DELAY_EDGE);
  }
  candidate_t c;
  c.valid = 1;
  c.strategy = (best_polarity < 0.0f && fabsf(refined_delay) < 0.25f) ? STRATEGY_POLARITY_FLIP : STRATEGY_FRACTIONAL_DELAY;
  c.delay_samples = refined_delay;
  c.polarity = best_polarity;
  c.correlation = best_corr;
  return c;
}

/* :539-636 */
static mix_diag_t mix_phase_safe_stereo(const float *x, size_t frame_count, float *mono, opt_f32 stereo_corr, phase_state_t *state) {
  mix_diag_t d = {STRATEGY_NONE, 0.0f, 0};
  const float current_correlation = stereo_corr.some ? stereo_corr.value : 1.0f;
  const candidate_t detected = best_phase_alignment(x, frame_count, current_correlation);
  if (detected.valid) {
    state->last_candidate = detected;
  } else if (current_correlation >= WARNING_CORRELATION) {
    if (state->last_candidate.valid) COUNT(CNT_HYSTERESIS_CLEARED);
    state->last_candidate.valid = 0;
  } else if (state->last_candidate.valid) {
    COUNT(CNT_HYSTERESIS_REUSED);
  }
  const candidate_t candidate = detected.valid ? detected : state->last_candidate;
  if (!candidate.valid) {
    if (current_correlation < WARNING_CORRELATION) {
      const size_t channel = strongest_channel_index(x, 2, frame_count);
      for (size_t f = 0; f < frame_count; ++f) mono[f] = x[2 * f + channel];
      d.strategy = STRATEGY_MAX_RMS_FALLBACK;
      COUNT(CNT_STRATEGY_FALLBACK);
      return d;
    }
    for (size_t f = 0; f < frame_count; ++f) {
      const float left = x[2 * f], right = x[2 * f + 1];
      mono[f] = 0.5f * (left + right);
    }
    COUNT(CNT_STRATEGY_NONE);
    return d;
  }

  const float c0 = candidate.correlation > 0.0f ? candidate.correlation : 0.0f;  /* f32::max(0.0) */
  const float mix_gain = clampf(1.0f / (2.0f * sqrtf(0.5f + 0.5f * c0)), 0.5f, FRAC_1_SQRT_2);
  COUNT(candidate.strategy == STRATEGY_POLARITY_FLIP ? CNT_STRATEGY_FLIP : CNT_STRATEGY_FRACTIONAL);
  for (size_t f = 0; f < frame_count; ++f) {
    const float left = x[2 * f], right = x[2 * f + 1];
    state_push(state, left, right);
    if (candidate.strategy == STRATEGY_POLARITY_FLIP) {
      mono[f] = (left + right * candidate.polarity) * mix_gain;
      continue;
    }
    const size_t required_history = (size_t)ceilf(LATENCY + fabsf(candidate.delay_samples)) + 2;
    if (state->filled <= required_history) {
      mono[f] = fabsf(left) >= fabsf(right) ? left : right;
      COUNT(CNT_WARM_UP);
      continue;
    }
    float aligned_left, aligned_right;
    if (candidate.delay_samples >= 0.0f) {
      aligned_left = lagrange_sample(state->left_history, LATENCY + candidate.delay_samples);
      aligned_right = lagrange_sample(state->right_history, LATENCY);
    } else {
      aligned_left = lagrange_sample(state->left_history, LATENCY);
      aligned_right = lagrange_sample(state->right_history, LATENCY - candidate.delay_samples);
    }
    mono[f] = (aligned_left + aligned_right * candidate.polarity) * mix_gain;
  }
  d.strategy = candidate.strategy;
  d.estimated_delay_samples = candidate.delay_samples;
  d.polarity_flipped = candidate.polarity < 0.0f;
  return d;
}

/* :659-736.  `n_samples` interleaved samples, `mono_len` slots; returns the frames written. */
static size_t mix_with_mode_and_state(const float *x, size_t n_samples, size_t num_channels, int mode, float *mono, size_t mono_len,
                                      phase_state_t *state, opt_f32 *corr_out, mix_diag_t *diag_out) {
  mix_diag_t d = {STRATEGY_NONE, 0.0f, 0};
  opt_f32 corr = {0, 0.0f};
  *diag_out = d;
  *corr_out = corr;
  if (num_channels == 0 || mono_len == 0) return 0;
  size_t frame_count = n_samples / num_channels;
  if (frame_count > mono_len) frame_count = mono_len;
  if (num_channels == 2) corr = stereo_correlation(x, frame_count);

  if (mode == MODE_LEFT) {
    for (size_t f = 0; f < frame_count; ++f) mono[f] = x[f * num_channels];
  } else if (mode == MODE_RIGHT) {
    const size_t channel = num_channels > 1 ? 1 : 0;
    for (size_t f = 0; f < frame_count; ++f) mono[f] = x[f * num_channels + channel];
  } else if (mode == MODE_MAX_RMS) {
    const size_t channel = strongest_channel_index(x, num_channels, frame_count);
    for (size_t f = 0; f < frame_count; ++f) mono[f] = x[f * num_channels + channel];
  } else if (mode == MODE_PHASE_SAFE_MONO && num_channels == 2) {
    d = mix_phase_safe_stereo(x, frame_count, mono, corr, state);
  } else {
    const float inv_channel_count = 1.0f / (float)num_channels;
    for (size_t f = 0; f < frame_count; ++f) {
      float sum = 0.0f;
      for (size_t c = 0; c < num_channels; ++c) sum += x[f * num_channels + c];
      mono[f] = sum * inv_channel_count;
    }
  }
  *corr_out = corr;
  *diag_out = d;
  return frame_count;
}

/* ------------------------------------------------------------------ exported */
mixdown_t *mdr_new(int n_channels, int mode) {
  mixdown_t *m = (mixdown_t *)calloc(1, sizeof *m);
  if (!m) return NULL;
  m->n_channels = n_channels;
  m->mode = mode;
  m->stereo_correlation = NAN;
  return m;
}
void mdr_free(mixdown_t *m) { free(m); }
void mdr_set_mode(mixdown_t *m, int mode) { m->mode = mode; }
int mdr_mode(const mixdown_t *m) { return m->mode; }

/* a fresh PhaseSafeMonoState and fresh diagnostics (a new input stream); the branch counters are kept */
void mdr_reset(mixdown_t *m) {
  memset(&m->state, 0, sizeof m->state);
  m->stereo_correlation = NAN;
  m->phase_warning_count = 0;
  m->strategy = STRATEGY_NONE;
  m->estimated_delay = 0.0f;
  m->polarity_flipped = 0;
}

/* the input callback, :789-842: `n_frames` interleaved frames in, as many mono frames out */
void mdr_callback(mixdown_t *m, const float *data, size_t n_frames, float *out) {
  t_cnt = m->counters;
  const size_t C = (size_t)m->n_channels;
  if (C == 1) {
    m->strategy = STRATEGY_NONE;
    m->estimated_delay = 0.0f;
    m->polarity_flipped = 0;
    memcpy(out, data, sizeof(float) * n_frames);
    t_cnt = NULL;
    return;
  }
  size_t frame_idx = 0;
  while (frame_idx < n_frames) {
    const size_t chunk_frames = n_frames - frame_idx < SCRATCH_CAPACITY ? n_frames - frame_idx : SCRATCH_CAPACITY;
    opt_f32 corr;
    mix_diag_t d;
    const size_t written = mix_with_mode_and_state(data + frame_idx * C, chunk_frames * C, C, m->mode, m->scratch, SCRATCH_CAPACITY,
                                                   &m->state, &corr, &d);
    m->strategy = d.strategy;
    m->estimated_delay = d.estimated_delay_samples;
    m->polarity_flipped = d.polarity_flipped;
    if (corr.some) {
      m->stereo_correlation = corr.value;
      if (corr.value < WARNING_CORRELATION) m->phase_warning_count++;
    }
    memcpy(out + frame_idx, m->scratch, sizeof(float) * written);
    frame_idx += chunk_frames;
  }
  t_cnt = NULL;
}

void mdr_diagnostics(const mixdown_t *m, float *stereo_correlation, uint64_t *phase_warning_count, int *strategy,
                     float *estimated_delay, int *polarity_flipped) {
  *stereo_correlation = m->stereo_correlation;
  *phase_warning_count = m->phase_warning_count;
  *strategy = m->strategy;
  *estimated_delay = m->estimated_delay;
  *polarity_flipped = m->polarity_flipped;
}

void mdr_counters(const mixdown_t *m, uint64_t *out) { memcpy(out, m->counters, sizeof m->counters); }
int mdr_counter_count(void) { return CNT_COUNT; }

/* the state, for tests: histories [2][16], filled, last_candidate (valid, strategy, delay, polarity, correlation) */
void mdr_state(const mixdown_t *m, float *history, int *filled, int *lc_valid, int *lc_strategy, float *lc) {
  memcpy(history, m->state.left_history, sizeof(float) * HISTORY);
  memcpy(history + HISTORY, m->state.right_history, sizeof(float) * HISTORY);
  *filled = (int)m->state.filled;
  *lc_valid = m->state.last_candidate.valid;
  *lc_strategy = m->state.last_candidate.strategy;
  lc[0] = m->state.last_candidate.delay_samples;
  lc[1] = m->state.last_candidate.polarity;
  lc[2] = m->state.last_candidate.correlation;
}

/* the stateless test entry (mix_interleaved_to_mono_with_mode, :639-657) and the one with a caller-kept state object */
size_t mdr_mix(mixdown_t *m, const float *x, size_t n_samples, float *mono, size_t mono_len, int *corr_some, float *corr,
               int *strategy, float *delay, int *flipped) {
  t_cnt = m->counters;
  opt_f32 c;
  mix_diag_t d;
  const size_t w = mix_with_mode_and_state(x, n_samples, (size_t)m->n_channels, m->mode, mono, mono_len, &m->state, &c, &d);
  t_cnt = NULL;
  *corr_some = c.some;
  *corr = c.value;
  *strategy = d.strategy;
  *delay = d.estimated_delay_samples;
  *flipped = d.polarity_flipped;
  return w;
}

float mdr_lagrange_sample(const float *history16, float delay) { return lagrange_sample(history16, delay); }
