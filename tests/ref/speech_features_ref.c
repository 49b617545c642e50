/* speech_features_ref.c -- the speech-feature measurement (python/mic_eq/analysis/voice_setup.py:161-458, 48 kHz) on the CPU, one
 * stream per call, for the tests: what csrc/af_speech_features.hip computes, restated operation by operation in the same
 * order (lane-strided sums with an xor tree, lfilter's transposed direct form II, the mixed-radix transform of 960 complex
 * points, band sums in bin order, medians by selection, the weighted sum one frame at a time), so that frame powers, chunk
 * energies, band sums, selected values and weighted sums carry the kernels' bits.  What the host does between the kernels
 * (levels, masks, loudness windows, the frame features and the frame model) is csrc/af_speech_features_math.h itself, which
 * the library shares: tests/test_speech_features_ref.py holds that text to the reference's recorded results, and
 * tests/test_gpu_speech_features.py holds the kernels to this file.  The recommendation rules behind the features
 * (csrc/af_voice_setup_math.h, voice_setup.py:1143-1223 and :468-696) are reached the same way.  Compiled unfused
 * (-ffp-contract=off). */
#define _GNU_SOURCE /* sincos */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../audio-forge_amd/csrc/af_speech_features_math.h"
#include "../../audio-forge_amd/csrc/af_voice_setup_math.h"

#define PI 3.14159265358979323846
#define N SFM_FRAME
#define M SFM_HOP
#define BANDS 6
#define SIB 5

static const int factors[8] = {5, 3, 2, 2, 2, 2, 2, 2}; /* 960, the largest radix first */
static const double band_low[BANDS] = {80.0, 250.0, 2000.0, 5000.0, 250.0, 5000.0};
static const double band_high[BANDS] = {250.0, 2000.0, 5000.0, 10000.0, 4500.0, 9500.0};
/* :133-136: b0 b1 b2 a1 a2 */
static const double shelf[5] = {1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585};
static const double highpass[5] = {1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621};

static double window[N], twiddles[2 * N], freqs[M + 1];
static int first[BANDS], last[BANDS], tables_made;

static void make_tables(void) {
  if (tables_made) return;
  for (int i = 0; i < N; ++i) window[i] = 0.5 + 0.5 * cos(PI * (double)(2 * i + 1 - N) / (double)(N - 1)); /* np.hanning */
  for (int k = 0; k < N; ++k) sincos(-2.0 * PI * (double)k / (double)N, &twiddles[2 * k + 1], &twiddles[2 * k]);
  {
    const double d = 1.0 / (double)SFM_RATE, val = 1.0 / ((double)N * d); /* np.fft.rfftfreq */
    for (int k = 0; k <= M; ++k) freqs[k] = (double)k * val;
  }
  for (int b = 0; b < BANDS; ++b) {
    first[b] = 0;
    last[b] = -1;
    for (int k = 0, seen = 0; k <= M; ++k)
      if (freqs[k] >= band_low[b] && freqs[k] <= band_high[b]) { if (!seen) { first[b] = k; seen = 1; } last[b] = k; }
  }
  tables_made = 1;
}

int sfr_sibilance_bins(void) { make_tables(); return last[SIB] - first[SIB] + 1; }
void sfr_sibilance_freqs(double *out) { make_tables(); memcpy(out, freqs + first[SIB], sizeof(double) * (size_t)(last[SIB] - first[SIB] + 1)); }

/* ---- the kernels' arithmetic ---- */
static double xor_tree(double *a /* [64] */) {
  double t[64];
  for (int off = 32; off >= 1; off >>= 1) {
    for (int l = 0; l < 64; ++l) t[l] = a[l] + a[l ^ off];
    memcpy(a, t, sizeof t);
  }
  return a[0];
}

static double frame_power(const float *x) { /* sf_frame_power_kernel */
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

static void kweight_energy(const float *x, int64_t n, double *energy) { /* sf_kweight_kernel */
  double a[2] = {0.0, 0.0}, h[2] = {0.0, 0.0}, acc = 0.0;
  int in_chunk = 0;
  int64_t chunk = 0;
  for (int64_t i = 0; i < n; ++i) {
    const double y = section(highpass, section(shelf, (double)x[i], a), h);
    acc += y * y;
    if (++in_chunk == M) { energy[chunk++] = acc; acc = 0.0; in_chunk = 0; }
  }
  if (in_chunk > 0) energy[chunk] = acc;
}

/* one radix-p stage over sub-transforms of length L; tw[2 * 2e], tw[2 * 2e + 1] = exp(-2 pi i e / M) */
static void stage(double *buf, int L, int p, const double *tw) {
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
          const double *t = tw + 2 * (2 * (((q * r) % p) * root));
          tr = ar[q] * t[0] - ai[q] * t[1];
          ti = ar[q] * t[1] + ai[q] * t[0];
        }
        accr = accr + tr;
        acci = acci + ti;
      }
      if (r != 0) {
        const double *t = tw + 2 * (2 * (j * r * scale));
        yr[r] = accr * t[0] - acci * t[1];
        yi[r] = accr * t[1] + acci * t[0];
      } else {
        yr[r] = accr;
        yi[r] = acci;
      }
    }
    for (int r = 0; r < p; ++r) { buf[2 * (base + r * Ls)] = yr[r]; buf[2 * (base + r * Ls) + 1] = yi[r]; }
  }
}

static int digit_reverse(int k) {
  int pos = 0, stride = M;
  for (int i = 0; i < 8; ++i) {
    stride /= factors[i];
    pos += (k % factors[i]) * stride;
    k /= factors[i];
  }
  return pos;
}

/* |rfft((x - mean) hanning)|^2 + 1e-18 of one frame, bins 0 .. 960 (sf_frame_kernel up to its row) */
static void frame_row(const float *x, double *p) {
  double part[256], total[4], mean, buf[N];
  for (int t = 0; t < 256; ++t) { /* np.mean(frame): strided partial sums, an xor tree per wave, the waves in order */
    double s = 0.0;
    for (int i = t; i < N; i += 256) s += (double)x[i];
    part[t] = s;
  }
  for (int w = 0; w < 4; ++w) total[w] = xor_tree(part + 64 * w);
  mean = (((total[0] + total[1]) + total[2]) + total[3]) / (double)N;
  for (int i = 0; i < N; ++i) buf[i] = ((double)x[i] - mean) * window[i];
  for (int i = 0, L = M; i < 8; ++i) {
    stage(buf, L, factors[i], twiddles);
    L /= factors[i];
  }
  for (int k = 0; k <= M; ++k) {
    const int ia = digit_reverse(k % M), ib = digit_reverse((M - k) % M);
    const double ax = buf[2 * ia], ay = buf[2 * ia + 1], bx = buf[2 * ib], by = buf[2 * ib + 1], tx = twiddles[2 * k], ty = twiddles[2 * k + 1];
    const double er = 0.5 * (ax + bx), ei = 0.5 * (ay - by);
    const double orr = 0.5 * (ay + by), oi = -0.5 * (ax - bx);
    const double xr = er + (orr * tx - oi * ty), xi = ei + (orr * ty + oi * tx);
    p[k] = (xr * xr + xi * xi) + 1e-18;
  }
}

static double band_sum(const double *p, int b) {
  double s = 0.0;
  for (int k = first[b]; k <= last[b]; ++k) s += p[k];
  return s;
}

/* lower and upper middle of v[0 .. n): what launch_vs_median and the rank selection of sf_frame_kernel leave */
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

/* One stream.  Arrays as af_speech_features_outputs, one stream's part; model: intercept | six coefficients, or NULL for the
 * published one.  Returns 0, or -1 for a capture below one frame. */
int sfr_analyze(const float *speech, int64_t n, double noise_rms_db, const double *vad, int64_t n_vad, const float *noise, int64_t m,
                const double *model, af_speech_features_row *row, double *frame_db, uint8_t *active_mask, int32_t *frame_indices,
                double *probabilities, double *features, double *power, double *energy, double *band, double *sib_mid, int32_t *sib_arg,
                double *sib_rows, double *noise_band, double *weighted, int32_t *weighted_arg) {
  double published[1 + SFM_FEATURES], p[M + 1];
  const int F = (int)sfm_frames(n), C = (int)sfm_chunks(n), Fn = noise ? (int)sfm_frames(m) : 0;
  if (n < N) return -1;
  make_tables();
  published[0] = SFM_FRAME_INTERCEPT;
  memcpy(published + 1, sfm_frame_coefficients, sizeof sfm_frame_coefficients);
  if (!model) model = published;
  memset(row, 0, sizeof *row);
  const int S = last[SIB] - first[SIB] + 1;

  for (int f = 0; f < F; ++f) power[f] = frame_power(speech + (int64_t)f * M);
  kweight_energy(speech, n, energy);
  if (!all_finite(power, F) || !all_finite(energy, C)) { row->non_finite = 1; return 0; }

  uint8_t *energy_active = (uint8_t *)malloc((size_t)F);
  double *post = (double *)malloc(sizeof(double) * (size_t)F), *weights = (double *)malloc(sizeof(double) * (size_t)F);
  sfm_masks(power, F, noise_rms_db, vad, n_vad, frame_db, energy_active, active_mask, post, frame_indices, row);
  sfm_loudness(energy, n, active_mask, F, row);
  const int A = row->spectral_frames;

  for (int i = 0; i < A; ++i) { /* sf_frame_kernel, a speech frame */
    frame_row(speech + (int64_t)frame_indices[i] * M, p);
    double *b = band + (size_t)i * SFM_BAND_FIELDS;
    const double *sib = p + first[SIB];
    for (int j = 0; j < BANDS; ++j) b[j] = band_sum(p, j);
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
    frame_row(noise + (int64_t)f * M, p);
    noise_band[f] = band_sum(p, SIB);
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
                 freqs + first[SIB], features, probabilities, weights, row);
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
      row->peak_hz = freqs[first[SIB] + best];
    }
  }
  free(weights);
  free(post);
  free(energy_active);
  return 0;
}

/* the rules of csrc/af_voice_setup_math.h for one stream */
void sfr_default_inputs(af_voice_setup_inputs *in) { vsm_default_inputs(in); }
void sfr_recommend(const af_voice_setup_inputs *in, af_voice_setup_recommendation *out) { vsm_recommend(in, out); }
