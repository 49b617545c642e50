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

/* the frame geometry of a rate and resample_poly's figures towards 48 kHz (sfm_make_geometry below) */
typedef struct sfm_geometry {
  int32_t rate, frame, hop, vad_window; /* int(fs 40 / 1000), int(fs 20 / 1000), ceil(fs 512 / 16000) */
  int32_t up, down;                     /* 48000 / g, fs / g with g = gcd(fs, 48000); 1, 1 at 48 kHz: no resampling */
  int32_t half, pre, rem, taps;         /* resample_poly: 10 max(up, down); zeros in front of the filter; first output; taps a phase */
} sfm_geometry;
static inline void sfm_masks_at(const sfm_geometry *g, const double *power, int F, double noise_rms_db, const double *vad, int64_t n_vad,
                                double *frame_db, uint8_t *energy_active, uint8_t *active, double *post, int32_t *listed,
                                af_speech_features_row *r);

/* :178-205 and :269-270 from the frame powers: frame levels, the adaptive floor, the energy mask, the posterior mask with its
 * six-frame rule, the three-frame dilation, and the list of spectrally active frames.  post: [F], written when vad is given. */
static inline void sfm_masks(const double *power, int F, double noise_rms_db, const double *vad, int64_t n_vad, double *frame_db,
                             uint8_t *energy_active, uint8_t *active, double *post, int32_t *listed, af_speech_features_row *r) {
  static const sfm_geometry at48 = {SFM_RATE, SFM_FRAME, SFM_HOP, SFM_VAD_WINDOW, 1, 1, 0, 0, 0, 0};
  sfm_masks_at(&at48, power, F, noise_rms_db, vad, n_vad, frame_db, energy_active, active, post, listed, r);
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

/* ---- device rates: the same measurement at 16, 22.05, 24, 32, 44.1, 48, 88.2 and 96 kHz.  Frames and masks live at the capture's
 * rate; the loudness lives at 48 kHz behind scipy.signal.resample_poly (voice_setup.py:127-140 and :214-230), on chunks of 960
 * resampled samples.  The 48 kHz forms above keep their names and results; at 48 kHz the forms below give the same bits. */
#define SFM_CHUNK48 960 /* the loudness grid: 20 ms at 48 kHz, whatever the capture's rate */
static const int32_t sfm_rates[8] = {16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000};


/* 0, or -1 for a rate outside the list */
static inline int sfm_make_geometry(int64_t rate, sfm_geometry *g) {
  int i, listed = 0;
  int64_t a, b;
  memset(g, 0, sizeof *g);
  for (i = 0; i < 8; ++i) listed |= rate == sfm_rates[i];
  if (!listed) return -1;
  g->rate = (int32_t)rate;
  g->frame = (int32_t)((double)rate * 40.0 / 1000.0);
  g->hop = (int32_t)((double)rate * 20.0 / 1000.0);
  g->vad_window = (int32_t)((rate * 512 + 15999) / 16000);
  for (a = rate, b = SFM_RATE; b;) { const int64_t t = a % b; a = b; b = t; }
  g->up = (int32_t)(SFM_RATE / a);
  g->down = (int32_t)(rate / a);
  if (g->up == g->down) return 0;
  g->half = 10 * (g->up > g->down ? g->up : g->down);
  g->pre = g->down - g->half % g->down;
  g->rem = (g->half + g->pre) / g->down;
  g->taps = (g->pre + 2 * g->half + 1 + g->up - 1) / g->up;
  return 0;
}

static inline int64_t sfm_frames_at(const sfm_geometry *g, int64_t n) { return n < g->frame ? 0 : (n - g->frame) / g->hop + 1; }
static inline int64_t sfm_chunks_at(const sfm_geometry *g, int64_t n) { return (n + g->hop - 1) / g->hop; }
/* the length resample_poly returns: ceil(n up / down) */
static inline int64_t sfm_resampled_length(const sfm_geometry *g, int64_t n) { return (n * g->up + g->down - 1) / g->down; }
static inline int64_t sfm_chunks48(const sfm_geometry *g, int64_t n) { return (sfm_resampled_length(g, n) + SFM_CHUNK48 - 1) / SFM_CHUNK48; }

/* scipy.special.i0 by its power series: sum of ((x / 2)^2)^k / (k!)^2 */
static inline double sfm_i0(double x) {
  const double q = (x / 2.0) * (x / 2.0);
  double term = 1.0, sum = 1.0;
  int k;
  for (k = 1; k < 200; ++k) {
    term = term * q / ((double)k * (double)k);
    sum += term;
    if (term < sum * 1e-17) break;
  }
  return sum;
}

/* resample_poly's default filter: firwin(2 half + 1, 1 / max(up, down), window=("kaiser", 5.0)) * up behind `pre` zeros, as the
 * polyphase table table[phase * taps + m] = hz[phase + m up] (0 behind the filter's end) */
static inline void sfm_polyphase_table(const sfm_geometry *g, double *table /* [up][taps] */) {
  const double pi = 3.14159265358979323846;
  const int N = 2 * g->half + 1;
  const double cutoff = 1.0 / (double)(g->up > g->down ? g->up : g->down), alpha = (double)g->half, i0_beta = sfm_i0(5.0);
  double *h = (double *)malloc(sizeof(double) * (size_t)N), sum = 0.0;
  int i, phase, m;
  for (i = 0; i < N; ++i) {
    const double t = (double)i - alpha, x = cutoff * t, ratio = t / alpha;
    const double sinc = x == 0.0 ? 1.0 : sin(pi * x) / (pi * x);
    h[i] = cutoff * sinc * (sfm_i0(5.0 * sqrt(1.0 - ratio * ratio)) / i0_beta);
    sum += h[i];
  }
  for (i = 0; i < N; ++i) h[i] = h[i] / sum * (double)g->up;
  for (phase = 0; phase < g->up; ++phase)
    for (m = 0; m < g->taps; ++m) {
      const int at = phase + m * g->up - g->pre;
      table[(size_t)phase * g->taps + m] = at >= 0 && at < N ? h[at] : 0.0;
    }
  free(h);
}

/* output o of resample_poly over x[0 .. n): the products of one phase, the oldest input first, multiplied and added apart */
#define SFM_POLYPHASE_SUM(g, table, n, o, VALUE, acc)                                       \
  do {                                                                                      \
    const int64_t t_ = ((int64_t)(o) + (g)->rem) * (g)->down, xi_ = t_ / (g)->up;           \
    const double *row_ = (table) + (size_t)(t_ % (g)->up) * (g)->taps;                      \
    int m_;                                                                                 \
    (acc) = 0.0;                                                                            \
    for (m_ = (g)->taps - 1; m_ >= 0; --m_) {                                               \
      const int64_t j = xi_ - m_;                                                           \
      if (j >= 0 && j < (n)) (acc) += (VALUE) * row_[m_];                                   \
    }                                                                                       \
  } while (0)

/* :178-205 at the capture's rate: sfm_masks with the geometry's hop, frame and posterior window */
static inline void sfm_masks_at(const sfm_geometry *g, const double *power, int F, double noise_rms_db, const double *vad, int64_t n_vad,
                                double *frame_db, uint8_t *energy_active, uint8_t *active, double *post, int32_t *listed,
                                af_speech_features_row *r) {
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
    af_interpolate_vad_probabilities(vad, n_vad, g->vad_window, F, g->hop, g->frame, xp, xp + n_vad, post);
    for (f = 0; f < F; ++f) {
      posterior[f] = (post[f] >= SFM_VAD_EVIDENCE && frame_db[f] >= low) || post[f] >= SFM_VAD_STRONG;
      count += posterior[f];
      evidence += post[f] >= SFM_VAD_EVIDENCE;
    }
    if (count >= 6) memcpy(active, posterior, (size_t)F);
    free(posterior);
    free(xp);
  }
  if (F >= 3) {
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

/* the sample mask at the capture's rate: sample j is active when frame j / hop or the one before it is (each covers two hops;
 * behind the last frame nothing is) */
static inline int sfm_sample_active(const sfm_geometry *g, const uint8_t *active, int F, int64_t j) {
  const int64_t f = j / g->hop;
  return (f < F && active[f]) || (f >= 1 && f - 1 < F && active[f - 1]);
}

/* one window size over the 48 kHz chunks, :143-158: count[c] of the W 960 samples of a window active, its K-weighted energy */
static inline int sfm_windows48(const double *energy, const int32_t *count, int64_t n48, int W, int H, double *out) {
  int n_out = 0;
  int64_t c0;
  for (c0 = 0; (c0 + W) * SFM_CHUNK48 <= n48; c0 += H) {
    int64_t masked = 0;
    int c;
    double sum = 0.0;
    for (c = 0; c < W; ++c) masked += count[c0 + c];
    if ((double)masked / (double)((int64_t)W * SFM_CHUNK48) < 0.55) continue;
    for (c = 0; c < W; ++c) sum += energy[c0 + c];
    out[n_out++] = sfm_lufs(sum / (double)((int64_t)W * SFM_CHUNK48));
  }
  return n_out;
}

/* :207-261 at a device rate.  energy, masked_energy, count: [sfm_chunks48(n)] -- sum(y^2), the same over the samples whose
 * resampled mask is >= 0.5, and how many those are, per chunk of 960 samples of the K-weighted 48 kHz signal of n48 samples.
 * At 48 kHz the caller derives the last two from the hop mask (sfm_chunk_mask48) and the results are sfm_loudness's. */
static inline void sfm_loudness_at(const sfm_geometry *g, const double *energy, const double *masked_energy, const int32_t *count,
                                   int64_t n, const uint8_t *active, int F, af_speech_features_row *r) {
  const int64_t n48 = sfm_resampled_length(g, n);
  const int C = (int)sfm_chunks48(g, n), Cr = (int)sfm_chunks_at(g, n);
  uint8_t *mask = (uint8_t *)calloc((size_t)Cr + 1, 1);
  double *momentary = (double *)malloc(sizeof(double) * (size_t)(C + 1)), *short_term = (double *)malloc(sizeof(double) * (size_t)(C + 1));
  double *sorted;
  int f, c, n_m, n_s;
  int64_t masked = 0;
  for (f = 0; f < F; ++f)
    if (active[f]) mask[f] = mask[f + 1] = 1;
  for (c = 0; c < Cr; ++c) masked += mask[c];
  r->active_duration_s = (double)(masked * g->hop) / (double)g->rate;
  r->active_ratio = (double)(masked * g->hop) / (double)n;
  n_m = sfm_windows48(energy, count, n48, 20, 5, momentary);
  n_s = sfm_windows48(energy, count, n48, 150, 50, short_term);
  if (n_m == 0) { /* the mean over the samples behind the resampled mask, :243-249 */
    double sum = 0.0;
    int64_t total = 0;
    for (c = 0; c < C; ++c)
      if (count[c]) { sum += masked_energy[c]; total += count[c]; }
    momentary[0] = sfm_lufs(total ? sum / (double)total : 0.0);
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

/* at 48 kHz the resampled mask is the hop mask itself: count and masked energy of every chunk from the active frames */
static inline void sfm_chunk_mask48(const double *energy, int64_t n, const uint8_t *active, int F, int32_t *count, double *masked_energy) {
  const int C = (int)sfm_chunks(n);
  int c;
  for (c = 0; c < C; ++c) {
    const int on = (c < F && active[c]) || (c >= 1 && c - 1 < F && active[c - 1]);
    count[c] = on ? SFM_CHUNK48 : 0;
    masked_energy[c] = on ? energy[c] : 0.0;
  }
}

/* the band edges of :271-276 and :305-308 at a rate: low[6], high[6] in the order of SFM_BAND_FIELDS */
static inline void sfm_band_edges(int64_t rate, double *low, double *high) {
  static const double lo[6] = {80.0, 250.0, 2000.0, 5000.0, 250.0, 5000.0}, hi[6] = {250.0, 2000.0, 5000.0, 10000.0, 4500.0, 9500.0};
  const double cap = (double)rate * 0.45;
  int b;
  for (b = 0; b < 6; ++b) { low[b] = lo[b]; high[b] = hi[b]; }
  if (cap < high[3]) high[3] = cap;
  if (cap < high[5]) high[5] = cap;
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
