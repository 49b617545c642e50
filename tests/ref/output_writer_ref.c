/* output_writer_ref.c -- the reference's output writer restated in C for the tests: OutputWriteContext::write_chunk
 * (rust-core/src/audio/processor/output_writer.rs:62-110) and what it calls, one object per stream, in front of a modelled
 * queue (capacity, fill; a write takes min(pending, free) frames).  The true-peak limiter and detector are the oracle's
 * afo_tp_* (this file is linked against the built oracle).  Built with -ffp-contract=off: every f32 operation is the
 * reference's, in its order.  Used by the tests only. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "af_oracle.h"

#define OWR_MAX_BLOCK 8672 /* the realtime scratches, dsp_loop.rs (OUTPUT_QUEUE_CONTROL / FADE / SAFETY capacities) */

enum {
  OWR_C_PASS_THROUGH, OWR_C_EXPANDED, OWR_C_COMPRESSED, OWR_C_EMERGENCY, OWR_C_OUT_LEN_ONE, OWR_C_MAX_SRC_CLAMP,
  OWR_C_FADE_CONTINUED, OWR_C_FADE_ENDED_INSIDE, OWR_C_SHORT_WRITE, OWR_C_ZERO_FREE, OWR_C_LIMITER_OFF, OWR_C_LIMITED,
  OWR_C_CLIP, OWR_C_NON_FINITE, OWR_C_COUNT
};

typedef struct {
  /* OutputWriteLimits, output_writer.rs:20-27 */
  size_t target_center, hard_backlog, fade_samples;
  float max_catchup_ratio, max_emergency_ratio;
  size_t capacity, scratch_capacity; /* the queue's and the retime scratch's */
  /* state */
  float drift_error_ema;
  size_t fade_remaining;
  afo_tp_limiter limiter;
  afo_tp_detector detector;
  int limiter_enabled;
  float ceiling_linear;
  float sample_rate;
  /* OutputWriteCounters, output_writer.rs:1-18 */
  uint64_t jitter_dropped, retime_adjustments, recovery_events, short_write_dropped, clip_events, true_peak_events;
  float clip_peak_db, true_peak_db, true_peak_input_db, gain_reduction_db, gain_reduction_history_db, headroom_db;
  uint32_t output_buffer_len;
  /* the last call: linear statistics and the decision */
  float in_true_peak, limiter_out_true_peak, detector_true_peak, min_gain, max_clipped;
  float ratio;
  size_t out_len, free_len, written;
  uint64_t branch[OWR_C_COUNT];
} owr;

/* resampling.rs:1-3 */
size_t owr_duration_samples(uint32_t sample_rate, uint32_t duration_ms) {
  uint64_t v = ((uint64_t)sample_rate * (uint64_t)duration_ms + 500u) / 1000u;
  return (size_t)(v < 1 ? 1 : v);
}

/* dsp_loop.rs:781-795 and :204 (the queue: two seconds of the output rate); processor.rs:66-68 */
void owr_default_limits(uint32_t rate, size_t *capacity, size_t *center, size_t *hard, size_t *fade) {
  size_t low = owr_duration_samples(rate, 30), high = owr_duration_samples(rate, 40);
  *center = (low + high + 1) / 2; /* div_ceil(2) */
  *hard = owr_duration_samples(rate, 60);
  size_t f = owr_duration_samples(rate, 6);
  *fade = f < 1 ? 1 : f;
  *capacity = 2 * (size_t)rate;
}

static void owr_fresh(owr *w) {
  /* dsp_loop.rs:796-802 and the atomics' initial values, processor.rs:659-668 */
  w->drift_error_ema = 0.0f;
  w->fade_remaining = 0;
  afo_tp_limiter_init(&w->limiter, w->sample_rate, -1.5f, 80.0f); /* default_settings, true_peak.rs:285-287 */
  afo_tp_detector_init(&w->detector);
  w->jitter_dropped = w->retime_adjustments = w->recovery_events = w->short_write_dropped = 0;
  w->clip_events = w->true_peak_events = 0;
  w->clip_peak_db = -120.0f;
  w->true_peak_db = -120.0f;
  w->true_peak_input_db = -120.0f;
  w->gain_reduction_db = 0.0f;
  w->gain_reduction_history_db = 0.0f;
  w->headroom_db = 120.0f;
  w->output_buffer_len = 0;
  w->in_true_peak = w->limiter_out_true_peak = w->detector_true_peak = w->max_clipped = 0.0f;
  w->min_gain = 1.0f;
  w->ratio = 1.0f;
  w->out_len = w->free_len = w->written = 0;
}

owr *owr_new(float sample_rate, size_t capacity, size_t center, size_t hard, size_t fade, size_t scratch_capacity) {
  owr *w = (owr *)calloc(1, sizeof(owr));
  w->sample_rate = sample_rate;
  w->capacity = capacity;
  w->target_center = center;
  w->hard_backlog = hard;
  w->fade_samples = fade;
  w->scratch_capacity = scratch_capacity ? scratch_capacity : OWR_MAX_BLOCK;
  w->max_catchup_ratio = 1.03f;   /* dsp_loop.rs:790 */
  w->max_emergency_ratio = 1.06f; /* dsp_loop.rs:791 */
  w->limiter_enabled = 1;
  w->ceiling_linear = 1.0f;
  owr_fresh(w);
  return w;
}
void owr_free(owr *w) { free(w); }
void owr_reset(owr *w) {
  owr_fresh(w);
  memset(w->branch, 0, sizeof(w->branch));
}
void owr_set_limiter(owr *w, int enabled, float ceiling_linear) {
  w->limiter_enabled = enabled;
  w->ceiling_linear = ceiling_linear;
}
void owr_set_state(owr *w, float ema, size_t fade_remaining) {
  w->drift_error_ema = ema;
  w->fade_remaining = fade_remaining;
}

static inline float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

/* resampling.rs:81-120.  Returns the output length; `out` holds it (a pass-through is copied). */
size_t owr_retime(const float *in, size_t n, float speed_ratio, size_t max_output_len, size_t scratch_capacity, float *out,
                  uint64_t *branch) {
  if (n == 0 || max_output_len == 0) return 0;
  const float clamped_ratio = fmaxf(speed_ratio, 0.5f);
  size_t desired_len = (size_t)fmaxf(roundf((float)n / clamped_ratio), 1.0f);
  size_t out_len = desired_len < max_output_len ? desired_len : max_output_len;
  if (scratch_capacity < out_len) out_len = scratch_capacity;
  if (out_len == n) {
    memcpy(out, in, sizeof(float) * n);
    if (branch) branch[OWR_C_PASS_THROUGH]++;
    return n;
  }
  if (branch) {
    branch[out_len > n ? OWR_C_EXPANDED : OWR_C_COMPRESSED]++;
    if (out_len == 1) branch[OWR_C_OUT_LEN_ONE]++;
  }
  const float max_src = (float)(n - 1);
  int clamped = 0;
  for (size_t i = 0; i < out_len; ++i) {
    float src_pos = 0.0f;
    if (out_len != 1) {
      const float p = (float)i * clamped_ratio;
      if (p > max_src) clamped = 1;
      src_pos = fminf(p, max_src);
    }
    const size_t idx0 = (size_t)floorf(src_pos);
    const size_t idx1 = idx0 + 1 < n - 1 ? idx0 + 1 : n - 1;
    const float frac = src_pos - (float)idx0;
    const float y0 = in[idx0], y1 = in[idx1];
    out[i] = y0 + (y1 - y0) * frac;
  }
  if (branch && clamped) branch[OWR_C_MAX_SRC_CLAMP]++;
  return out_len;
}

/* routing.rs:651-655 */
void owr_update_decaying_peak_db(float value_db, float *history, float decay_db_per_update) {
  const float previous = fmaxf(*history, 0.0f);
  const float decayed = fmaxf(previous - fmaxf(decay_db_per_update, 0.0f), 0.0f);
  *history = fmaxf(value_db, decayed);
}

/* routing.rs:768-799 */
void owr_sanitize_and_clamp(float *buf, size_t n, float ceiling_linear, uint64_t *clip_events, float *clip_peak_db,
                            float *max_clipped_out) {
  const float ceiling = clampf(ceiling_linear, 0.0f, 1.0f);
  uint64_t clipped = 0;
  float max_clipped = 0.0f;
  for (size_t i = 0; i < n; ++i) {
    if (!isfinite(buf[i])) {
      buf[i] = 0.0f;
      continue;
    }
    const float amplitude = fabsf(buf[i]);
    if (amplitude > ceiling) {
      clipped++;
      max_clipped = fmaxf(max_clipped, amplitude);
    }
    buf[i] = clampf(buf[i], -ceiling, ceiling);
  }
  if (clipped > 0) {
    *clip_events += clipped;
    const float peak_db = 20.0f * log10f(max_clipped);
    if (peak_db > *clip_peak_db) *clip_peak_db = peak_db;
  }
  if (max_clipped_out) *max_clipped_out = max_clipped;
}

/* output_writer.rs:62-110.  `fill` frames are in the queue at the call.  Returns the frames written (0 for an empty
 * block: the reference returns false and touches nothing); `out` (OWR_MAX_BLOCK floats) holds them. */
size_t owr_write_chunk(owr *w, const float *src, size_t n, size_t fill, int clean_path, float *out) {
  if (n == 0) return 0;
  static _Thread_local float a[OWR_MAX_BLOCK];
  const size_t capacity = w->capacity;
  const size_t free_len = capacity - fill;
  size_t len = n;
  if (len > OWR_MAX_BLOCK) len = OWR_MAX_BLOCK; /* (the callers keep blocks to 8192 frames) */
  w->ratio = 1.0f;
  if (!clean_path) {
    /* apply_drift_retime, :112-159 */
    const float error = (float)fill - (float)w->target_center;
    w->drift_error_ema = w->drift_error_ema * 0.85f + error * 0.15f;
    size_t pz = w->hard_backlog > w->target_center ? w->hard_backlog - w->target_center : 0;
    const float positive_zone = (float)(pz < 1 ? 1 : pz);
    const float negative_zone = (float)(w->target_center < 1 ? 1 : w->target_center);
    const float normalized_error = w->drift_error_ema >= 0.0f ? clampf(w->drift_error_ema / positive_zone, 0.0f, 1.0f)
                                                              : clampf(w->drift_error_ema / negative_zone, -1.0f, 0.0f);
    float ratio = clampf(1.0f + normalized_error * 0.008f, 0.96f, w->max_catchup_ratio); /* processor.rs:69-70 */
    if (fill >= w->hard_backlog) {
      ratio = w->max_emergency_ratio;
      w->branch[OWR_C_EMERGENCY]++;
    }
    w->ratio = ratio;
    const size_t cap1 = capacity < 1 ? 1 : capacity;
    len = owr_retime(src, n, ratio, cap1, w->scratch_capacity, a, w->branch);
    if (len != n) {
      if (len < n) w->jitter_dropped += n - len;
      w->retime_adjustments += 1;
    }
    /* apply_discontinuity_fade, :161-192 */
    const size_t fade_remaining = w->fade_remaining;
    if (fade_remaining != 0 && len != 0) {
      const size_t fade_count = fade_remaining < len ? fade_remaining : len;
      const size_t elapsed = w->fade_samples > fade_remaining ? w->fade_samples - fade_remaining : 0;
      const float fade_total = (float)w->fade_samples;
      for (size_t i = 0; i < fade_count; ++i) a[i] *= clampf((float)(elapsed + i + 1) / fade_total, 0.0f, 1.0f);
      w->fade_remaining = fade_remaining - fade_count;
      if (elapsed > 0) w->branch[OWR_C_FADE_CONTINUED]++;
      if (w->fade_remaining == 0 && fade_count < len) w->branch[OWR_C_FADE_ENDED_INSIDE]++;
    }
  } else {
    memcpy(a, src, sizeof(float) * len);
  }
  /* sanitize_and_limit, :194-242 */
  const float output_ceiling = w->limiter_enabled ? w->ceiling_linear : 1.0f;
  int scrubbed = 0;
  for (size_t i = 0; i < len; ++i)
    if (!isfinite(a[i])) { /* routing.rs:697-703 */
      a[i] = 0.0f;
      scrubbed = 1;
    }
  if (scrubbed) w->branch[OWR_C_NON_FINITE]++;
  if (w->limiter_enabled) {
    afo_tp_limiter_set_ceiling_linear(&w->limiter, output_ceiling);
    /* process_block_inplace (true_peak.rs:337-378), a frame at a time so that the gain of every frame is seen */
    int limited = 0;
    float in_tp = 0.0f, out_tp = 0.0f, max_gr = 0.0f, min_gain = INFINITY;
    for (size_t i = 0; i < len; ++i) {
      afo_tp_block_stats st = afo_tp_limiter_process_block(&w->limiter, &a[i], 1);
      limited |= st.limited_events != 0;
      in_tp = fmaxf(in_tp, st.input_true_peak);
      out_tp = fmaxf(out_tp, st.output_true_peak);
      max_gr = fmaxf(max_gr, st.max_gain_reduction_db);
      min_gain = fminf(min_gain, w->limiter.gain_reduction);
    }
    w->in_true_peak = in_tp;
    w->limiter_out_true_peak = out_tp;
    w->min_gain = min_gain;
    /* record_true_peak_limiter_stats, :261-288 */
    if (limited) {
      w->true_peak_events += 1;
      w->branch[OWR_C_LIMITED]++;
    }
    w->true_peak_input_db = 20.0f * log10f(fmaxf(in_tp, 1e-10f));
    w->gain_reduction_db = max_gr;
    owr_update_decaying_peak_db(max_gr, &w->gain_reduction_history_db, 0.15f);
    w->headroom_db = 20.0f * log10f(fmaxf(output_ceiling, 1e-10f) / fmaxf(out_tp, 1e-10f));
  } else {
    afo_tp_limiter_reset(&w->limiter);
    w->gain_reduction_db = 0.0f;
    owr_update_decaying_peak_db(0.0f, &w->gain_reduction_history_db, 0.15f);
    w->in_true_peak = 0.0f;
    w->limiter_out_true_peak = 0.0f;
    w->min_gain = 1.0f;
    w->branch[OWR_C_LIMITER_OFF]++;
  }
  const uint64_t clips_before = w->clip_events;
  owr_sanitize_and_clamp(a, len, output_ceiling, &w->clip_events, &w->clip_peak_db, &w->max_clipped);
  if (w->clip_events != clips_before) w->branch[OWR_C_CLIP]++;
  /* record_true_peak, :244-259 */
  const float true_peak = afo_tp_detector_process_block(&w->detector, a, len);
  w->detector_true_peak = true_peak;
  w->true_peak_db = 20.0f * log10f(fmaxf(true_peak, 1e-10f));
  w->headroom_db = 20.0f * log10f(fmaxf(output_ceiling, 1e-10f) / fmaxf(true_peak, 1e-10f));
  /* write_to_output_queue, :290-331, on the modelled queue */
  size_t pending = len;
  if (pending > free_len) {
    w->short_write_dropped += pending - free_len;
    w->recovery_events += 1;
    w->fade_remaining = w->fade_samples;
    pending = free_len;
    w->branch[OWR_C_SHORT_WRITE]++;
    if (free_len == 0) w->branch[OWR_C_ZERO_FREE]++;
  }
  memcpy(out, a, sizeof(float) * pending);
  /* update_output_fill, :333-343 */
  w->output_buffer_len = (uint32_t)(fill + pending);
  w->out_len = len;
  w->free_len = free_len;
  w->written = pending;
  return pending;
}

/* ---- read-outs */
int owr_branch_count(void) { return OWR_C_COUNT; }
void owr_branches(const owr *w, uint64_t *out) { memcpy(out, w->branch, sizeof(w->branch)); }
/* jitter_dropped, retime_adjustments, recovery_events, short_write_dropped, clip_events, true_peak_events */
void owr_counters(const owr *w, uint64_t *out) {
  out[0] = w->jitter_dropped;
  out[1] = w->retime_adjustments;
  out[2] = w->recovery_events;
  out[3] = w->short_write_dropped;
  out[4] = w->clip_events;
  out[5] = w->true_peak_events;
}
/* db[6]: clip_peak, true_peak, true_peak_input, gain_reduction, gain_reduction_history, headroom
 * lin[5]: input true peak, limiter output true peak, detector true peak, minimum gain, maximum clipped amplitude
 * rec[4]: out_len, fade_remaining, fill after the write, free at the call */
void owr_meters(const owr *w, float *db, float *lin, float *ratio, float *ema, int64_t *rec) {
  db[0] = w->clip_peak_db;
  db[1] = w->true_peak_db;
  db[2] = w->true_peak_input_db;
  db[3] = w->gain_reduction_db;
  db[4] = w->gain_reduction_history_db;
  db[5] = w->headroom_db;
  lin[0] = w->in_true_peak;
  lin[1] = w->limiter_out_true_peak;
  lin[2] = w->detector_true_peak;
  lin[3] = w->min_gain;
  lin[4] = w->max_clipped;
  *ratio = w->ratio;
  *ema = w->drift_error_ema;
  rec[0] = (int64_t)w->out_len;
  rec[1] = (int64_t)w->fade_remaining;
  rec[2] = (int64_t)w->output_buffer_len;
  rec[3] = (int64_t)w->free_len;
}
/* gain, the 20-frame delay line and its write index, and the three 32-tap histories (limiter in, limiter out, detector) */
void owr_state(const owr *w, float *gain, float *delay, int32_t *write_idx, float *hist) {
  *gain = w->limiter.gain_reduction;
  memcpy(delay, w->limiter.delay, sizeof(float) * AFO_TP_LOOKAHEAD);
  *write_idx = (int32_t)w->limiter.write_idx;
  memcpy(hist, w->limiter.in_os.history, sizeof(float) * AFO_TP_TAPS);
  memcpy(hist + AFO_TP_TAPS, w->limiter.out_os.history, sizeof(float) * AFO_TP_TAPS);
  memcpy(hist + 2 * AFO_TP_TAPS, w->detector.os.history, sizeof(float) * AFO_TP_TAPS);
}
