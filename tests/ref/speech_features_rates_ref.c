/* speech_features_rates_ref.c -- the speech-feature measurement at device rates (python/mic_eq/analysis/voice_setup.py:161-458 at
 * 16, 22.05, 24, 32, 44.1, 48, 88.2 and 96 kHz) on the CPU, one stream per call, for the tests: what csrc/af_speech_features.hip
 * computes behind af_device_rate_features_*, restated operation by operation in the same order.  It is speech_features_ref.c
 * with the frame geometry as data -- frame, hop, factor list, window, twiddles and band table of the rate -- and, in front of
 * the K-weighting, sf_resample_kernel: scipy.signal.resample_poly's polyphase sum of the capture and of its sample mask, the
 * oldest input first, multiplied and added apart, on the table of csrc/af_speech_features_math.h (which the library shares, as
 * it shares the host half: levels, masks, loudness windows, frame features and the frame model).  Compiled unfused
 * (-ffp-contract=off). */
#define _GNU_SOURCE /* sincos */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../audio-forge_amd/csrc/af_speech_features_math.h"

#define PI 3.14159265358979323846
#define BANDS 6
#define SIB 5
#define THREADS 256

/* :133-136: b0 b1 b2 a1 a2 */
static const double shelf[5] = {1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585};
static const double highpass[5] = {1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621};

typedef struct tables {
  sfm_geometry g;
  int n_factors, factor[16], first[BANDS], last[BANDS];
  double *window, *twiddles, *freqs, *phase; /* [frame], [2 frame], [hop + 1], [up][taps] or null */
} tables;

static tables made[8];

static const tables *tables_of(int64_t rate) {
  static const int radices[4] = {7, 5, 3, 2};
  double low[BANDS], high[BANDS];
  tables *t = NULL;
  for (int i = 0; i < 8; ++i)
    if (sfm_rates[i] == rate) t = &made[i];
  if (!t) return NULL;
  if (t->window) return t;
  sfm_make_geometry(rate, &t->g);
  const int N = t->g.frame, M = t->g.hop;
  for (int i = 0, left = M; i < 4; ++i) /* the largest radix first */
    while (left % radices[i] == 0) { t->factor[t->n_factors++] = radices[i]; left /= radices[i]; }
  t->twiddles = (double *)malloc(sizeof(double) * 2 * (size_t)N);
  t->freqs = (double *)malloc(sizeof(double) * (size_t)(M + 1));
  for (int k = 0; k < N; ++k) sincos(-2.0 * PI * (double)k / (double)N, &t->twiddles[2 * k + 1], &t->twiddles[2 * k]);
  {
    const double d = 1.0 / (double)rate, val = 1.0 / ((double)N * d); /* np.fft.rfftfreq */
    for (int k = 0; k <= M; ++k) t->freqs[k] = (double)k * val;
  }
  sfm_band_edges(rate, low, high);
  for (int b = 0; b < BANDS; ++b) {
    t->first[b] = 0;
    t->last[b] = -1;
    for (int k = 0, seen = 0; k <= M; ++k)
      if (t->freqs[k] >= low[b] && t->freqs[k] <= high[b]) { if (!seen) { t->first[b] = k; seen = 1; } t->last[b] = k; }
  }
  if (t->g.up != t->g.down) {
    t->phase = (double *)malloc(sizeof(double) * (size_t)t->g.up * t->g.taps);
    sfm_polyphase_table(&t->g, t->phase);
  }
  t->window = (double *)malloc(sizeof(double) * (size_t)N); /* last: its presence means "made" */
  for (int i = 0; i < N; ++i) t->window[i] = 0.5 + 0.5 * cos(PI * (double)(2 * i + 1 - N) / (double)(N - 1)); /* np.hanning */
  return t;
}

/* rate | frame | hop | vad_window | up | down | half | pre | rem | taps; -1 for a rate outside the list */
int sfq_geometry(int64_t rate, int32_t *out) {
  sfm_geometry g;
  if (sfm_make_geometry(rate, &g)) return -1;
  memcpy(out, &g, sizeof g);
  return 0;
}
int64_t sfq_frames(int64_t rate, int64_t n) { const tables *t = tables_of(rate); return t ? sfm_frames_at(&t->g, n) : -1; }
int64_t sfq_chunks(int64_t rate, int64_t n) { const tables *t = tables_of(rate); return t ? sfm_chunks48(&t->g, n) : -1; }
int64_t sfq_resampled_length(int64_t rate, int64_t n) { const tables *t = tables_of(rate); return t ? sfm_resampled_length(&t->g, n) : -1; }
int sfq_sibilance_bins(int64_t rate) { const tables *t = tables_of(rate); return t ? t->last[SIB] - t->first[SIB] + 1 : -1; }
void sfq_sibilance_freqs(int64_t rate, double *out) {
  const tables *t = tables_of(rate);
  memcpy(out, t->freqs + t->first[SIB], sizeof(double) * (size_t)(t->last[SIB] - t->first[SIB] + 1));
}
/* the polyphase table [up][taps]; -1 at 48 kHz */
int sfq_phase_table(int64_t rate, double *out) {
  const tables *t = tables_of(rate);
  if (!t || !t->phase) return -1;
  memcpy(out, t->phase, sizeof(double) * (size_t)t->g.up * t->g.taps);
  return 0;
}

/* ---- the kernels' arithmetic ---- */
static double xor_tree(double *a /* [64] */) {
  double t[64];
  for (int off = 32; off >= 1; off >>= 1) {
    for (int l = 0; l < 64; ++l) t[l] = a[l] + a[l ^ off];
    memcpy(a, t, sizeof t);
  }
  return a[0];
}

static double frame_power(const float *x, int N) { /* sf_frame_power_kernel */
  double q[64];
  for (int l = 0; l < 64; ++l) {
    double s = 0.0;
    for (int i = l; i < N; i += 64) s += (double)x[i] * (double)x[i];
    q[l] = s;
  }
  return xor_tree(q) / (double)N;
}

static double section(const double *c, double x, double *z) { /* lfilter, a0 = 1 */
  const double y = z[0] + c[0] * x;
  z[0] = (z[1] + c[1] * x) - c[3] * y;
  z[1] = c[2] * x - c[4] * y;
  return y;
}

/* sf_resample_kernel over one stream: y[n48], mask[n48] (resampled sample mask >= 0.5), counts per chunk of 960 */
static void resample(const tables *t, const float *x, int64_t n, const uint8_t *active, int F, double *y, uint8_t *mask, int32_t *counts) {
  const sfm_geometry *g = &t->g;
  const int64_t n48 = sfm_resampled_length(g, n);
  memset(counts, 0, sizeof(int32_t) * (size_t)sfm_chunks48(g, n));
  for (int64_t o = 0; o < n48; ++o) {
    double acc, macc;
    SFM_POLYPHASE_SUM(g, t->phase, n, o, (double)x[j], acc);
    SFM_POLYPHASE_SUM(g, t->phase, n, o, (sfm_sample_active(g, active, F, j) ? 1.0 : 0.0), macc);
    y[o] = acc;
    mask[o] = macc >= 0.5;
    counts[o / SFM_CHUNK48] += mask[o];
  }
}

/* sf_kweight_kernel<double, true>: chunk energies of the K-weighted signal, and the same behind the mask */
static void kweight_energy48(const double *x, const uint8_t *mask, int64_t n, double *energy, double *masked_energy) {
  double a[2] = {0.0, 0.0}, h[2] = {0.0, 0.0}, acc = 0.0, macc = 0.0;
  int in_chunk = 0;
  int64_t chunk = 0;
  for (int64_t i = 0; i < n; ++i) {
    const double y = section(highpass, section(shelf, x[i], a), h);
    acc += y * y;
    if (mask[i]) macc += y * y;
    if (++in_chunk == SFM_CHUNK48) { energy[chunk] = acc; masked_energy[chunk++] = macc; acc = macc = 0.0; in_chunk = 0; }
  }
  if (in_chunk > 0) { energy[chunk] = acc; masked_energy[chunk] = macc; }
}

static void kweight_energy(const float *x, int64_t n, double *energy) { /* sf_kweight_kernel<float, false> */
  double a[2] = {0.0, 0.0}, h[2] = {0.0, 0.0}, acc = 0.0;
  int in_chunk = 0;
  int64_t chunk = 0;
  for (int64_t i = 0; i < n; ++i) {
    const double y = section(highpass, section(shelf, (double)x[i], a), h);
    acc += y * y;
    if (++in_chunk == SFM_CHUNK48) { energy[chunk++] = acc; acc = 0.0; in_chunk = 0; }
  }
  if (in_chunk > 0) energy[chunk] = acc;
}

/* one radix-p stage over sub-transforms of length L; tw[2 * 2e], tw[2 * 2e + 1] = exp(-2 pi i e / M) */
static void stage(double *buf, int M, int L, int p, const double *tw) {
  const int Ls = L / p, root = M / p, scale = M / L;
  double ar[7], ai[7], yr[7], yi[7];
  for (int b = 0; b < M / p; ++b) {
    const int j = b % Ls, base = (b / Ls) * L + j;
    for (int q = 0; q < p; ++q) { ar[q] = buf[2 * (base + q * Ls)]; ai[q] = buf[2 * (base + q * Ls) + 1]; }
    for (int r = 0; r < p; ++r) {
      double accr = ar[0], acci = ai[0];
      for (int q = 1; q < p; ++q) {
        double tr = ar[q], ti = ai[q];
        if (r != 0) {
          const double *w = tw + 2 * (2 * (((q * r) % p) * root));
          tr = ar[q] * w[0] - ai[q] * w[1];
          ti = ar[q] * w[1] + ai[q] * w[0];
        }
        accr = accr + tr;
        acci = acci + ti;
      }
      if (r != 0) {
        const double *w = tw + 2 * (2 * (j * r * scale));
        yr[r] = accr * w[0] - acci * w[1];
        yi[r] = accr * w[1] + acci * w[0];
      } else {
        yr[r] = accr;
        yi[r] = acci;
      }
    }
    for (int r = 0; r < p; ++r) { buf[2 * (base + r * Ls)] = yr[r]; buf[2 * (base + r * Ls) + 1] = yi[r]; }
  }
}

static int digit_reverse(const tables *t, int k) {
  int pos = 0, stride = t->g.hop;
  for (int i = 0; i < t->n_factors; ++i) {
    stride /= t->factor[i];
    pos += (k % t->factor[i]) * stride;
    k /= t->factor[i];
  }
  return pos;
}

/* |rfft((x - mean) hanning)|^2 + 1e-18 of one frame, bins 0 .. hop (sf_frame_kernel up to its row) */
static void frame_row(const tables *t, const float *x, double *p, double *buf /* [frame] */) {
  const int N = t->g.frame, M = t->g.hop;
  double part[THREADS], total[4], mean;
  for (int i = 0; i < THREADS; ++i) { /* np.mean(frame): strided partial sums, an xor tree per wave, the waves in order */
    double s = 0.0;
    for (int k = i; k < N; k += THREADS) s += (double)x[k];
    part[i] = s;
  }
  for (int w = 0; w < 4; ++w) total[w] = xor_tree(part + 64 * w);
  mean = (((total[0] + total[1]) + total[2]) + total[3]) / (double)N;
  for (int i = 0; i < N; ++i) buf[i] = ((double)x[i] - mean) * t->window[i];
  for (int i = 0, L = M; i < t->n_factors; ++i) {
    stage(buf, M, L, t->factor[i], t->twiddles);
    L /= t->factor[i];
  }
  for (int k = 0; k <= M; ++k) {
    const int ia = digit_reverse(t, k % M), ib = digit_reverse(t, (M - k) % M);
    const double ax = buf[2 * ia], ay = buf[2 * ia + 1], bx = buf[2 * ib], by = buf[2 * ib + 1], tx = t->twiddles[2 * k], ty = t->twiddles[2 * k + 1];
    const double er = 0.5 * (ax + bx), ei = 0.5 * (ay - by);
    const double orr = 0.5 * (ay + by), oi = -0.5 * (ax - bx);
    const double xr = er + (orr * tx - oi * ty), xi = ei + (orr * ty + oi * tx);
    p[k] = (xr * xr + xi * xi) + 1e-18;
  }
}

static double band_sum(const tables *t, const double *p, int b) {
  double s = 0.0;
  for (int k = t->first[b]; k <= t->last[b]; ++k) s += p[k];
  return s;
}

static void middles(const double *v, int n, double *lower, double *upper) {
  double *s = sfm_sorted_copy(v, n);
  *lower = s[(n - 1) / 2];
  *upper = s[n / 2];
  free(s);
}

static int all_finite(const double *v, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (!isfinite(v[i])) return 0;
  return 1;
}

/* the resampling stage alone, for given frame flags [frames]: what af_device_rate_features_debug_resample_host leaves */
int sfq_resample(int64_t rate, const float *x, int64_t n, const uint8_t *active, double *y, uint8_t *mask, int32_t *counts) {
  const tables *t = tables_of(rate);
  if (!t || !t->phase) return -1;
  resample(t, x, n, active, (int)sfm_frames_at(&t->g, n), y, mask, counts);
  return 0;
}

/* One stream at `rate`.  Arrays as af_speech_features_outputs, one stream's part, with F, C and S of the rate; resampled [n48],
 * resampled_mask [n48], counts [C] and masked_energy [C] are what the resampling left (untouched at 48 kHz); model: intercept |
 * six coefficients, or NULL for the published one.  Returns 0, -1 for a capture below one frame, -2 for a rate outside the list. */
int sfq_analyze(int64_t rate, const float *speech, int64_t n, double noise_rms_db, const double *vad, int64_t n_vad, const float *noise,
                int64_t m, const double *model, af_speech_features_row *row, double *frame_db, uint8_t *active_mask, int32_t *frame_indices,
                double *probabilities, double *features, double *power, double *energy, double *band, double *sib_mid, int32_t *sib_arg,
                double *sib_rows, double *noise_band, double *weighted, int32_t *weighted_arg, double *resampled, uint8_t *resampled_mask,
                int32_t *counts, double *masked_energy) {
  const tables *t = tables_of(rate);
  if (!t) return -2;
  const sfm_geometry *g = &t->g;
  const int N = g->frame, M = g->hop;
  double published[1 + SFM_FEATURES];
  const int F = (int)sfm_frames_at(g, n), C = (int)sfm_chunks48(g, n), Fn = noise ? (int)sfm_frames_at(g, m) : 0;
  if (n < N) return -1;
  published[0] = SFM_FRAME_INTERCEPT;
  memcpy(published + 1, sfm_frame_coefficients, sizeof sfm_frame_coefficients);
  if (!model) model = published;
  memset(row, 0, sizeof *row);
  const int S = t->last[SIB] - t->first[SIB] + 1;

  for (int f = 0; f < F; ++f) power[f] = frame_power(speech + (int64_t)f * M, N);
  if (!all_finite(power, F)) { row->non_finite = 1; return 0; }
  uint8_t *energy_active = (uint8_t *)malloc((size_t)F);
  double *post = (double *)malloc(sizeof(double) * (size_t)F), *weights = (double *)malloc(sizeof(double) * (size_t)F);
  double *p = (double *)malloc(sizeof(double) * (size_t)(M + 1)), *buf = (double *)malloc(sizeof(double) * (size_t)N);
  sfm_masks_at(g, power, F, noise_rms_db, vad, n_vad, frame_db, energy_active, active_mask, post, frame_indices, row);
  if (t->phase) {
    resample(t, speech, n, active_mask, F, resampled, resampled_mask, counts);
    kweight_energy48(resampled, resampled_mask, sfm_resampled_length(g, n), energy, masked_energy);
  } else {
    kweight_energy(speech, n, energy);
  }
  if (!all_finite(energy, C)) {
    memset(row, 0, sizeof *row);
    row->non_finite = 1;
    goto done;
  }
  if (t->phase) sfm_loudness_at(g, energy, masked_energy, counts, n, active_mask, F, row);
  else sfm_loudness(energy, n, active_mask, F, row);
  const int A = row->spectral_frames;

  for (int i = 0; i < A; ++i) { /* sf_frame_kernel, a speech frame */
    frame_row(t, speech + (int64_t)frame_indices[i] * M, p, buf);
    double *b = band + (size_t)i * SFM_BAND_FIELDS;
    const double *sib = p + t->first[SIB];
    for (int j = 0; j < BANDS; ++j) b[j] = band_sum(t, p, j);
    int arg = 0;
    for (int k = 1; k < S; ++k)
      if (sib[k] > sib[arg]) arg = k;
    b[6] = sib[arg];
    b[7] = 0.0;
    sib_arg[i] = arg;
    middles(sib, S, &sib_mid[2 * i], &sib_mid[2 * i + 1]);
    memcpy(sib_rows + (size_t)i * S, sib, sizeof(double) * (size_t)S);
  }
  for (int f = 0; f < Fn; ++f) { /* ... a noise frame */
    frame_row(t, noise + (int64_t)f * M, p, buf);
    noise_band[f] = band_sum(t, p, SIB);
  }
  if (Fn && !all_finite(noise_band, Fn)) {
    memset(row, 0, sizeof *row);
    row->non_finite = 1;
  } else {
    double band_mid[2 * SFM_BAND_FIELDS] = {0}, noise_mid[2] = {0.0, 0.0};
    double *column = (double *)malloc(sizeof(double) * (size_t)(A > Fn ? A : Fn) + 8);
    for (int j = 0; j < SFM_BAND_FIELDS && A; ++j) { /* launch_vs_median over the listed frames */
      for (int i = 0; i < A; ++i) column[i] = band[(size_t)i * SFM_BAND_FIELDS + j];
      middles(column, A, &band_mid[j], &band_mid[SFM_BAND_FIELDS + j]);
    }
    if (Fn) middles(noise_band, Fn, &noise_mid[0], &noise_mid[1]);
    free(column);
    sfm_evidence(model, A, frame_indices, band, sib_mid, sib_arg, row->vad_probability_used ? post : NULL, band_mid, Fn, noise_mid,
                 t->freqs + t->first[SIB], features, probabilities, weights, row);
    if (A) { /* sf_weighted_peak_kernel */
      int best = 0;
      for (int k = 0; k < S; ++k) {
        double acc = 0.0;
        for (int i = 0; i < A; ++i) acc += weights[i] * sib_rows[(size_t)i * S + k];
        weighted[k] = acc;
      }
      for (int k = 1; k < S; ++k)
        if (weighted[k] > weighted[best]) best = k;
      *weighted_arg = best;
      row->peak_hz = t->freqs[t->first[SIB] + best];
    }
  }
done:
  free(buf);
  free(p);
  free(weights);
  free(post);
  free(energy_active);
  return 0;
}

/* the 48 kHz geometry through the rate-taking forms of the header, for the test that holds them to the old ones: masks and
 * loudness of one stream from its frame powers and chunk energies, both ways; returns 0 when every bit of the two rows agrees */
int sfq_forms_agree_at_48k(const double *power, int F, const double *energy, int64_t n, double noise_rms_db, const double *vad, int64_t n_vad) {
  sfm_geometry g;
  af_speech_features_row a, b;
  const int C = (int)sfm_chunks(n);
  int differ;
  double *db = (double *)malloc(sizeof(double) * (size_t)(4 * F + 2 * C + 2)), *post = db + F, *db2 = post + F, *post2 = db2 + F, *masked = post2 + F;
  uint8_t *flags = (uint8_t *)malloc((size_t)4 * F + 4);
  int32_t *listed = (int32_t *)malloc(sizeof(int32_t) * (size_t)(2 * F + C + 2)), *count = listed + 2 * F;
  memset(&a, 0, sizeof a);
  memset(&b, 0, sizeof b);
  sfm_make_geometry(SFM_RATE, &g);
  differ = g.frame != SFM_FRAME || g.hop != SFM_HOP || g.vad_window != SFM_VAD_WINDOW || g.up != 1 || g.down != 1 ||
           sfm_frames_at(&g, n) != sfm_frames(n) || sfm_chunks48(&g, n) != sfm_chunks(n) || sfm_chunks_at(&g, n) != sfm_chunks(n) ||
           sfm_resampled_length(&g, n) != n;
  sfm_masks(power, F, noise_rms_db, vad, n_vad, db, flags, flags + F, post, listed, &a);
  sfm_masks_at(&g, power, F, noise_rms_db, vad, n_vad, db2, flags + 2 * F, flags + 3 * F, post2, listed + F, &b);
  differ |= memcmp(db, db2, sizeof(double) * (size_t)F) || memcmp(flags, flags + 2 * F, (size_t)2 * F) ||
            memcmp(listed, listed + F, sizeof(int32_t) * (size_t)a.spectral_frames);
  sfm_loudness(energy, n, flags + F, F, &a);
  sfm_chunk_mask48(energy, n, flags + 3 * F, F, count, masked);
  sfm_loudness_at(&g, energy, masked, count, n, flags + 3 * F, F, &b);
  differ |= memcmp(&a, &b, sizeof a) != 0;
  free(listed);
  free(flags);
  free(db);
  return differ;
}
