/* CPU restatement of the room-noise reference analysis (test infrastructure only).
 *
 * Restates python/mic_eq/analysis/noise_reference.py:118-546 (_frame_analysis, _interpolate_vad, _quality_mean,
 * _select_in_capture_noise, analyze_noise_reference), one stream per call.  Metadata arrives as the library takes it: the
 * capture age and the mismatch bits of _metadata_mismatches.
 *
 * Where the reference calls NumPy (np.mean, np.fft.rfft, np.median over frames) this file uses the arithmetic of
 * csrc/af_noise_reference.hip instead, operation for operation: sums over 64 strided partials and an xor tree, a mixed-radix
 * decimation-in-frequency complex transform of half the frame length (largest radix first, every butterfly output summed in
 * index order) with the real-input split behind it, band sums in bin order, twiddles and the Hann window from the same f64
 * formulas the library uploads.  tests/test_noise_reference_ref.py holds it to the reference's recorded outputs within a
 * measured tolerance; the GPU tests then hold the kernels to it bit for bit.
 *
 * Build with -ffp-contract=off and without fast-math (tests/noise_reference_oracle.py does). */
#define _GNU_SOURCE /* sincos */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define PI 3.14159265358979323846
#define MIN_NOISE_DURATION_S 1.5   /* noise_reference.py:12 */
#define QUESTIONABLE_AGE_S 120.0   /* :13 */
#define INVALID_AGE_S 600.0        /* :14 */
#define VAD_CONTAMINATION 0.35     /* analysis/vad.py */
#define BANDS 7                    /* OCTAVE_CENTERS_HZ, :15-18 */
#define MAX_FACTORS 16

typedef struct nrr_row {
  int32_t status, conservative;
  uint32_t reasons, guidance;
  double quality_score;
  double duration_s, finite_fraction, noise_rms_db, conservative_noise_rms_db, noise_peak_db, crest_factor_db;
  double clipped_fraction, zero_fraction, rms_spread_db, octave_stability_db, spectral_flux_db;
  double vad_contamination_ratio, vad_contamination_p90, capture_age_s, in_capture_level_delta_db, spectral_shape_distance_db;
  double noise_sum_squares, noise_peak;
  int64_t finite_samples, clipped_samples, zero_samples;
  int32_t in_capture_noise_frame_count, noise_frames, speech_frames, n_bands, has_in_capture_spectrum, reserved;
} nrr_row;

/* ---- tables: the formulas of af_noise_reference_host.hpp ---- */
int nrr_frame_size(int fs) {  /* max(512, int(round(fs * 0.20))), :119 */
  const double r = nearbyint((double)fs * 0.20);
  return r < 512.0 ? 512 : (int)r;
}

int nrr_plan(int M, int *factor) {  /* the factor count, or -1 with a prime factor above 7 */
  static const int radices[4] = {7, 5, 3, 2};
  int n = 0;
  for (int i = 0; i < 4; ++i)
    while (M % radices[i] == 0 && n < MAX_FACTORS) { factor[n++] = radices[i]; M /= radices[i]; }
  return M == 1 ? n : -1;
}

static void make_window(int N, double *w, double *sumw2) {  /* np.hanning */
  double s = 0.0;
  for (int i = 0; i < N; ++i) {
    w[i] = 0.5 + 0.5 * cos(PI * (double)(2 * i + 1 - N) / (double)(N - 1));
    s += w[i] * w[i];
  }
  *sumw2 = s > 1e-18 ? s : 1e-18;
}

static void make_twiddles(int N, double *tw /* [N][2] */) {
  for (int k = 0; k < N; ++k) {
    const double a = -2.0 * PI * (double)k / (double)N;
    sincos(a, &tw[2 * k + 1], &tw[2 * k]);
  }
}

void nrr_freqs(int fs, int n, double *f) {  /* np.fft.rfftfreq(n, 1 / fs) */
  const double d = 1.0 / (double)fs, val = 1.0 / ((double)n * d);
  for (int k = 0; k <= n / 2; ++k) f[k] = (double)k * val;
}

static int make_bands(int fs, const double *freqs, int K, int *first, int *last) {  /* :138-145 */
  static const double centres[BANDS] = {125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0, 8000.0};
  int n = 0;
  for (int b = 0; b < BANDS; ++b) {
    const double low = centres[b] / sqrt(2.0), up = centres[b] * sqrt(2.0), cap = (double)fs * 0.49;
    const double high = up < cap ? up : cap;
    int f0 = -1, f1 = -1;
    for (int k = 0; k < K; ++k)
      if (freqs[k] >= low && freqs[k] < high) { if (f0 < 0) f0 = k; f1 = k; }
    if (f0 < 0) continue;
    first[n] = f0;
    last[n] = f1;
    ++n;
  }
  return n;
}

/* ---- the kernels' arithmetic ---- */
static double sample(const float *x, int64_t i) { return isfinite(x[i]) ? (double)x[i] : 0.0; }

static double xor_tree(double *a /* [64] */) {
  double t[64];
  for (int off = 32; off >= 1; off >>= 1) {
    for (int l = 0; l < 64; ++l) t[l] = a[l] + a[l ^ off];
    memcpy(a, t, sizeof t);
  }
  return a[0];
}

static void sample_stats(const float *x, int64_t n, nrr_row *r) {
  double q[64], peak = 0.0;
  int64_t finite = 0, clipped = 0, zero = 0;
  for (int l = 0; l < 64; ++l) {
    double s = 0.0;
    for (int64_t i = l; i < n; i += 64) {
      const double v = sample(x, i), a = fabs(v);
      finite += isfinite(x[i]) != 0;
      s += v * v;
      if (a > peak) peak = a;
      clipped += a >= 0.999;
      zero += a <= 1e-12;
    }
    q[l] = s;
  }
  r->noise_sum_squares = xor_tree(q);
  r->noise_peak = peak;
  r->finite_samples = finite;
  r->clipped_samples = clipped;
  r->zero_samples = zero;
}

static void chunk_sums(const float *x, int hop, double *sx, double *sxx) {
  double a[64], q[64];
  for (int l = 0; l < 64; ++l) {
    double s = 0.0, ss = 0.0;
    for (int i = l; i < hop; i += 64) {
      const double v = sample(x, i);
      s += v;
      ss += v * v;
    }
    a[l] = s;
    q[l] = ss;
  }
  *sx = xor_tree(a);
  *sxx = xor_tree(q);
}

static double frame_power(const float *x, int N, double mean) {
  double q[64];
  for (int l = 0; l < 64; ++l) {
    double s = 0.0;
    for (int i = l; i < N; i += 64) {
      const double d = sample(x, i) - mean;
      s += d * d;
    }
    q[l] = s;
  }
  return xor_tree(q) / (double)N;
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

static int digit_reverse(int k, int M, const int *factor, int n_factors) {
  int pos = 0, stride = M;
  for (int i = 0; i < n_factors; ++i) {
    stride /= factor[i];
    pos += (k % factor[i]) * stride;
    k /= factor[i];
  }
  return pos;
}

/* |rfft((x - mean) w)|^2 / sumw2 of one frame, bins 0 .. N / 2 */
static void frame_psd(const float *x, double mean, int N, const int *factor, int n_factors, const double *w, const double *tw,
                      double sumw2, double *buf /* [N] */, double *p) {
  const int M = N / 2;
  for (int i = 0; i < N; ++i) buf[i] = (sample(x, i) - mean) * w[i];
  for (int i = 0, L = M; i < n_factors; ++i) {
    stage(buf, M, L, factor[i], tw);
    L /= factor[i];
  }
  for (int k = 0; k <= M; ++k) {
    const int ia = digit_reverse(k % M, M, factor, n_factors), ib = digit_reverse((M - k) % M, M, factor, n_factors);
    const double ax = buf[2 * ia], ay = buf[2 * ia + 1], bx = buf[2 * ib], by = buf[2 * ib + 1], tx = tw[2 * k], ty = tw[2 * k + 1];
    const double er = 0.5 * (ax + bx), ei = 0.5 * (ay - by);
    const double orr = 0.5 * (ay + by), oi = -0.5 * (ax - bx);
    const double xr = er + (orr * tx - oi * ty), xi = ei + (orr * ty + oi * tx);
    p[k] = (xr * xr + xi * xi) / sumw2;
  }
}

/* ---- the host's arithmetic ---- */
static int cmp_double(const void *a, const void *b) {
  const double x = *(const double *)a, y = *(const double *)b;
  return (x > y) - (x < y);
}

static double percentile(const double *v, int n, double q) {  /* np.percentile "linear" */
  double *s = malloc(sizeof(double) * (size_t)n);
  memcpy(s, v, sizeof(double) * (size_t)n);
  qsort(s, (size_t)n, sizeof(double), cmp_double);
  const double idx = (q / 100.0) * (double)(n - 1);
  int lo = (int)floor(idx);
  if (lo < 0) lo = 0;
  if (lo > n - 1) lo = n - 1;
  const int hi = lo + 1 < n - 1 ? lo + 1 : n - 1;
  const double t = idx - (double)lo, a = s[lo], b = s[hi], diff = b - a;
  free(s);
  return t >= 0.5 ? b - diff * (1.0 - t) : a + diff * t;
}

static double median(const double *v, int n) {
  double *s = malloc(sizeof(double) * (size_t)n);
  memcpy(s, v, sizeof(double) * (size_t)n);
  qsort(s, (size_t)n, sizeof(double), cmp_double);
  const double m = n % 2 ? s[n / 2] : (s[n / 2 - 1] + s[n / 2]) / 2.0;
  free(s);
  return m;
}

static double clip(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }
static double db(double power) { return 10.0 * log10(fmax(power, 1e-18)); }

static double interp(double x, const double *xp, const double *fp, int n) {
  if (x < xp[0]) return fp[0];
  if (x >= xp[n - 1]) return fp[n - 1];
  int lo = 0, hi = n - 1;
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (x >= xp[mid]) lo = mid; else hi = mid;
  }
  const double slope = (fp[lo + 1] - fp[lo]) / (xp[lo + 1] - xp[lo]);
  return slope * (x - xp[lo]) + fp[lo];
}

static double *interpolate_vad(const double *vad, int64_t n_vad, int frames) {  /* :188-205; NULL for None */
  if (!vad || n_vad <= 0 || frames <= 0) return NULL;
  double *xp = malloc(sizeof(double) * (size_t)n_vad), *fp = malloc(sizeof(double) * (size_t)n_vad);
  double *out = malloc(sizeof(double) * (size_t)frames);
  for (int64_t i = 0; i < n_vad; ++i) {
    xp[i] = ((double)i + 0.5) / (double)n_vad;
    fp[i] = clip(vad[i], 0.0, 1.0);
  }
  for (int f = 0; f < frames; ++f) out[f] = interp(((double)f + 0.5) / (double)frames, xp, fp, (int)n_vad);
  free(xp);
  free(fp);
  return out;
}

static double sum8(const double *a) { return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7])); }

/* the middles of every column of rows[list[i]][K] and their dB median */
static void column_median(const double *rows, const int *list, int n, int K, double *middles /* [2][K], nullable */, double *out_db) {
  double *col = malloc(sizeof(double) * (size_t)n);
  for (int k = 0; k < K; ++k) {
    for (int i = 0; i < n; ++i) col[i] = rows[(size_t)list[i] * K + k];
    qsort(col, (size_t)n, sizeof(double), cmp_double);
    const double a = col[(n - 1) / 2], b = col[n / 2];
    if (middles) { middles[k] = a; middles[K + k] = b; }
    const double lo = db(a), hi = b == a ? lo : db(b);
    out_db[k] = (lo + hi) / 2.0;
  }
  free(col);
}

/* Outputs as af_noise_reference_outputs for one stream; every array is caller-allocated, spectra on the returned grid
 * (nrr_bins), the rest on the frame grid.  speech_psd: [Fv][K], every voice frame (the library transforms the quiet ones only).
 * Returns 0, or -1 for a frame size the transform does not take. */
int nrr_analyze(const float *noise, int64_t n_noise, const float *speech, int64_t n_speech, const double *noise_vad, int64_t n_noise_vad,
                const double *speech_vad, int64_t n_speech_vad, double age, uint32_t mismatch, int fs, nrr_row *r, double *explicit_out,
                double *conservative_out, double *in_capture_out, double *frame_rms_out, double *band_levels_out, double *chunk_sums_out,
                double *noise_power_out, double *speech_power_out, double *noise_psd_out, double *band_power_out,
                double *explicit_middles, double *in_capture_middles, uint8_t *quiet_mask_out) {
  const int N = nrr_frame_size(fs), M = N / 2, K = M + 1, hop = M;
  int factor[MAX_FACTORS];
  const int n_factors = N % 2 ? -1 : nrr_plan(M, factor);
  if (n_factors < 0) return -1;
  const int Fn = n_noise < N ? 0 : (int)((n_noise - N) / hop) + 1;
  const int Fs = (!speech || n_speech < N) ? 0 : (int)((n_speech - N) / hop) + 1;
  double *w = malloc(sizeof(double) * (size_t)N), *tw = malloc(sizeof(double) * 2 * (size_t)N), *buf = malloc(sizeof(double) * (size_t)N);
  double *freqs = malloc(sizeof(double) * (size_t)K), sumw2;
  int first[BANDS], last[BANDS];
  make_window(N, w, &sumw2);
  make_twiddles(N, tw);
  nrr_freqs(fs, N, freqs);
  const int NB = make_bands(fs, freqs, K, first, last);
  const int grid_n = Fn ? N : (int)(n_noise > 2 ? n_noise : 2), Ko = grid_n / 2 + 1;
  double *grid = malloc(sizeof(double) * (size_t)Ko);
  nrr_freqs(fs, grid_n, grid);
  const double nan = NAN;

  memset(r, 0, sizeof *r);
  sample_stats(noise, n_noise, r);

  /* both captures: chunk sums, centred frame powers */
  double *nsum = malloc(sizeof(double) * 2 * (size_t)(Fn + 1)), *ssum = malloc(sizeof(double) * 2 * (size_t)(Fs + 1));
  double *npow = malloc(sizeof(double) * (size_t)(Fn + 1)), *spow = malloc(sizeof(double) * (size_t)(Fs + 1));
  double *nrms = malloc(sizeof(double) * (size_t)(Fn + 1)), *srms = malloc(sizeof(double) * (size_t)(Fs + 1));
  if (Fn) for (int c = 0; c <= Fn; ++c) chunk_sums(noise + (int64_t)c * hop, hop, &nsum[2 * c], &nsum[2 * c + 1]);
  if (Fs) for (int c = 0; c <= Fs; ++c) chunk_sums(speech + (int64_t)c * hop, hop, &ssum[2 * c], &ssum[2 * c + 1]);
  for (int f = 0; f < Fn; ++f) {
    npow[f] = frame_power(noise + (int64_t)f * hop, N, (nsum[2 * f] + nsum[2 * f + 2]) / (double)N);
    nrms[f] = db(npow[f]);
  }
  for (int f = 0; f < Fs; ++f) {
    spow[f] = frame_power(speech + (int64_t)f * hop, N, (ssum[2 * f] + ssum[2 * f + 2]) / (double)N);
    srms[f] = db(spow[f]);
  }
  if (chunk_sums_out && Fn) memcpy(chunk_sums_out, nsum, sizeof(double) * 2 * (size_t)(Fn + 1));
  if (noise_power_out) memcpy(noise_power_out, npow, sizeof(double) * (size_t)Fn);
  if (speech_power_out) memcpy(speech_power_out, spow, sizeof(double) * (size_t)Fs);
  if (frame_rms_out) memcpy(frame_rms_out, nrms, sizeof(double) * (size_t)Fn);

  /* the noise frames: PSD rows, band sums, the column median */
  double *npsd = malloc(sizeof(double) * (size_t)(Fn + 1) * K), *bandp = malloc(sizeof(double) * (size_t)(Fn + 1) * BANDS);
  double *explicit_db = malloc(sizeof(double) * (size_t)K), *in_capture_db = malloc(sizeof(double) * (size_t)K);
  int *list = malloc(sizeof(int) * (size_t)(Fn + Fs + 1));
  for (int f = 0; f < Fn; ++f) {
    double *p = npsd + (size_t)f * K;
    frame_psd(noise + (int64_t)f * hop, (nsum[2 * f] + nsum[2 * f + 2]) / (double)N, N, factor, n_factors, w, tw, sumw2, buf, p);
    for (int b = 0; b < BANDS; ++b) bandp[(size_t)f * BANDS + b] = 0.0;
    for (int b = 0; b < NB; ++b) {
      double s = 0.0;
      for (int k = first[b]; k <= last[b]; ++k) s += p[k];
      bandp[(size_t)f * BANDS + b] = s;
    }
    list[f] = f;
  }
  if (noise_psd_out) memcpy(noise_psd_out, npsd, sizeof(double) * (size_t)Fn * K);
  if (band_power_out) memcpy(band_power_out, bandp, sizeof(double) * (size_t)Fn * BANDS);
  if (Fn) column_median(npsd, list, Fn, K, explicit_middles, explicit_db);

  /* _select_in_capture_noise, :252-277 */
  int quiet_count = 0, selected = 0;
  double in_capture_rms_db = 0.0;
  if (quiet_mask_out) memset(quiet_mask_out, 0, (size_t)Fs);
  if (Fs >= 4) {
    double *post = interpolate_vad(speech_vad, n_speech_vad, Fs);
    int go = 1;
    if (post) {
      const double threshold = percentile(srms, Fs, 35.0);
      for (int f = 0; f < Fs; ++f)
        if (post[f] <= 0.25 && srms[f] <= threshold) list[quiet_count++] = f;
      free(post);
    } else {
      const double spread = percentile(srms, Fs, 90.0) - percentile(srms, Fs, 10.0);
      if (spread < 6.0) go = 0;
      else {
        const double threshold = percentile(srms, Fs, 15.0);
        for (int f = 0; f < Fs; ++f)
          if (srms[f] <= threshold) list[quiet_count++] = f;
      }
    }
    const int minimum = (int)ceil((double)Fs * 0.05) > 3 ? (int)ceil((double)Fs * 0.05) : 3;
    if (go && quiet_count >= minimum) {
      selected = 1;
      double *kept = malloc(sizeof(double) * (size_t)quiet_count), *qpsd = malloc(sizeof(double) * (size_t)quiet_count * K);
      int *ql = malloc(sizeof(int) * (size_t)quiet_count);
      for (int i = 0; i < quiet_count; ++i) {
        const int f = list[i];
        kept[i] = srms[f];
        ql[i] = i;
        if (quiet_mask_out) quiet_mask_out[f] = 1;
        frame_psd(speech + (int64_t)f * hop, (ssum[2 * f] + ssum[2 * f + 2]) / (double)N, N, factor, n_factors, w, tw, sumw2, buf,
                  qpsd + (size_t)i * K);
      }
      in_capture_rms_db = median(kept, quiet_count);
      column_median(qpsd, ql, quiet_count, K, in_capture_middles, in_capture_db);
      free(kept);
      free(qpsd);
      free(ql);
    }
  }
  if (!selected && in_capture_middles)
    for (int k = 0; k < 2 * K; ++k) in_capture_middles[k] = nan;
  if (!Fn && explicit_middles)
    for (int k = 0; k < 2 * K; ++k) explicit_middles[k] = nan;

  /* analyze_noise_reference, :294-546 */
  const double n = (double)n_noise;
  uint32_t reasons = 0, guidance = 0;
  int invalid = 0, questionable = 0;
  const double finite_fraction = n_noise ? (double)r->finite_samples / n : 0.0;
  const double duration_s = n / (double)fs;
  const double noise_rms_db = db(n_noise ? r->noise_sum_squares / n : 0.0);
  const double noise_peak_db = 20.0 * log10(fmax(n_noise ? r->noise_peak : 0.0, 1e-9));
  const double crest_factor_db = fmax(0.0, noise_peak_db - noise_rms_db);
  const double clipped_fraction = n_noise ? (double)r->clipped_samples / n : 0.0;
  const double zero_fraction = n_noise ? (double)r->zero_samples / n : 1.0;
  if (duration_s < MIN_NOISE_DURATION_S) { invalid = 1; reasons |= 1u << 0; guidance |= 1u << 0; }
  if (finite_fraction < 1.0) { invalid = 1; reasons |= 1u << 1; guidance |= 1u << 1; }
  if (noise_rms_db <= -95.0 || (zero_fraction >= 0.995 && noise_peak_db <= -90.0)) { invalid = 1; reasons |= 1u << 2; guidance |= 1u << 2; }
  if (clipped_fraction > 0.001) { invalid = 1; reasons |= 1u << 3; guidance |= 1u << 3; }
  else if (clipped_fraction > 0.0) { questionable = 1; reasons |= 1u << 4; guidance |= 1u << 4; }

  double rms_spread_db = 120.0, octave_stability_db = 120.0, spectral_flux_db = 120.0;
  if (Fn == 0) {
    invalid = 1;
    reasons |= 1u << 5;
    for (int k = 0; k < Ko; ++k) explicit_out[k] = -120.0;
  } else {
    memcpy(explicit_out, explicit_db, sizeof(double) * (size_t)K);
    rms_spread_db = percentile(nrms, Fn, 90.0) - percentile(nrms, Fn, 10.0);
    octave_stability_db = 0.0;
    spectral_flux_db = 0.0;
    if (band_levels_out)
      for (int i = 0; i < Fn * BANDS; ++i) band_levels_out[i] = nan;
    if (NB > 0) {
      double *levels = malloc(sizeof(double) * (size_t)Fn * NB), *column = malloc(sizeof(double) * (size_t)Fn);
      double spread[BANDS], row[BANDS];
      for (int f = 0; f < Fn; ++f)
        for (int b = 0; b < NB; ++b) {
          levels[f * NB + b] = db(bandp[(size_t)f * BANDS + b]);
          if (band_levels_out) band_levels_out[f * BANDS + b] = levels[f * NB + b];
        }
      for (int b = 0; b < NB; ++b) {
        for (int f = 0; f < Fn; ++f) column[f] = levels[f * NB + b];
        spread[b] = percentile(column, Fn, 90.0) - percentile(column, Fn, 10.0);
      }
      octave_stability_db = median(spread, NB);
      if (Fn >= 2) {
        double *normalized = malloc(sizeof(double) * (size_t)Fn * NB), *flux = malloc(sizeof(double) * (size_t)(Fn - 1));
        for (int f = 0; f < Fn; ++f) {
          const double mid = median(&levels[f * NB], NB);
          for (int b = 0; b < NB; ++b) normalized[f * NB + b] = levels[f * NB + b] - mid;
        }
        for (int f = 0; f + 1 < Fn; ++f) {
          for (int b = 0; b < NB; ++b) row[b] = fabs(normalized[(f + 1) * NB + b] - normalized[f * NB + b]);
          flux[f] = median(row, NB);
        }
        spectral_flux_db = percentile(flux, Fn - 1, 95.0);
        free(normalized);
        free(flux);
      }
      free(levels);
      free(column);
    }
    if (rms_spread_db > 12.0 || octave_stability_db > 14.0) { invalid = 1; reasons |= 1u << 6; guidance |= 1u << 5; }
    else if (rms_spread_db > 6.0 || octave_stability_db > 8.0) { questionable = 1; reasons |= 1u << 7; guidance |= 1u << 6; }
    if (spectral_flux_db > 10.0) { invalid = 1; reasons |= 1u << 8; guidance |= 1u << 7; }
    else if (spectral_flux_db > 6.0 || crest_factor_db > 24.0) { questionable = 1; reasons |= 1u << 9; guidance |= 1u << 7; }
  }

  double vad_ratio = 0.0, vad_p90 = 0.0;
  double *post = interpolate_vad(noise_vad, n_noise_vad, Fn);
  if (post) {
    int above = 0;
    for (int f = 0; f < Fn; ++f) above += post[f] >= VAD_CONTAMINATION;
    vad_ratio = (double)above / (double)Fn;
    vad_p90 = percentile(post, Fn, 90.0);
    free(post);
  }
  if (vad_ratio > 0.30) { invalid = 1; reasons |= 1u << 10; guidance |= 1u << 8; }
  else if (vad_ratio > 0.08 || vad_p90 > 0.55) { questionable = 1; reasons |= 1u << 11; guidance |= 1u << 9; }

  if (mismatch & 0x3fu) { invalid = 1; reasons |= (mismatch & 0x3fu) << 12; guidance |= 1u << 10; }
  const int have_age = !isnan(age);
  const double capture_age_s = have_age ? fmax(0.0, age) : nan;
  if (have_age) {
    if (capture_age_s > INVALID_AGE_S) { invalid = 1; reasons |= 1u << 18; guidance |= 1u << 11; }
    else if (capture_age_s > QUESTIONABLE_AGE_S) { questionable = 1; reasons |= 1u << 19; guidance |= 1u << 12; }
  }

  double level_delta_db = nan, shape_distance_db = nan, conservative_rms_db = noise_rms_db;
  memcpy(conservative_out, explicit_out, sizeof(double) * (size_t)Ko);
  if (selected) {
    for (int k = 0; k < Ko; ++k) in_capture_out[k] = Fn ? in_capture_db[k] : interp(grid[k], freqs, in_capture_db, K);
    level_delta_db = in_capture_rms_db - noise_rms_db;
    int any = 0, count = 0;
    for (int k = 0; k < Ko; ++k) any = any || (grid[k] >= 80.0 && grid[k] <= 8000.0);
    double *e = malloc(sizeof(double) * (size_t)Ko), *c = malloc(sizeof(double) * (size_t)Ko);
    for (int k = 0; k < Ko; ++k)
      if (!any || (grid[k] >= 80.0 && grid[k] <= 8000.0)) { e[count] = explicit_out[k]; c[count] = in_capture_out[k]; ++count; }
    const double me = median(e, count), mc = median(c, count);
    for (int i = 0; i < count; ++i) e[i] = fabs((e[i] - me) - (c[i] - mc));
    shape_distance_db = median(e, count);
    free(e);
    free(c);
    for (int k = 0; k < Ko; ++k) conservative_out[k] = fmax(explicit_out[k], in_capture_out[k]);
    conservative_rms_db = fmax(noise_rms_db, in_capture_rms_db);
    if (level_delta_db > 12.0 || shape_distance_db > 10.0) { invalid = 1; reasons |= 1u << 20; guidance |= 1u << 13; }
    else if (level_delta_db > 6.0 || shape_distance_db > 5.5) { questionable = 1; reasons |= 1u << 21; guidance |= 1u << 14; }
    else if (level_delta_db < -20.0) { invalid = 1; reasons |= 1u << 22; guidance |= 1u << 15; }
    else if (level_delta_db < -12.0) { questionable = 1; reasons |= 1u << 23; guidance |= 1u << 16; }
  } else {
    for (int k = 0; k < Ko; ++k) in_capture_out[k] = nan;
  }

  double consistency = 1.0;
  if (selected) {
    consistency *= clip(1.0 - fmax(0.0, level_delta_db) / 12.0, 0.0, 1.0);
    consistency *= clip(1.0 - shape_distance_db / 10.0, 0.0, 1.0);
  }
  const double values[8] = {clip(duration_s / 3.0, 0.0, 1.0),
                            clip((finite_fraction - 0.995) / 0.005, 0.0, 1.0),
                            clip(1.0 - rms_spread_db / 12.0, 0.0, 1.0),
                            clip(1.0 - octave_stability_db / 14.0, 0.0, 1.0),
                            clip(1.0 - fmax(0.0, crest_factor_db - 12.0) / 18.0, 0.0, 1.0),
                            clip(1.0 - vad_ratio / 0.30, 0.0, 1.0),
                            consistency,
                            have_age ? clip(1.0 - capture_age_s / INVALID_AGE_S, 0.0, 1.0) : 1.0};
  double weights[8] = {0.10, 0.10, 0.18, 0.15, 0.10, 0.15, 0.17, 0.05}, terms[8];
  const double total = sum8(weights);
  for (int i = 0; i < 8; ++i) {
    weights[i] /= total;
    terms[i] = weights[i] * log(fmax(clip(values[i], 0.0, 1.0), 0.02));
  }
  double quality = exp(sum8(terms));
  if (invalid) quality = fmin(quality, 0.20);
  else if (questionable) quality = fmin(quality, 0.64);

  r->status = invalid ? 2 : (questionable ? 1 : 0);
  r->conservative = questionable || invalid || selected;
  r->reasons = reasons;
  r->guidance = guidance;
  r->quality_score = clip(quality, 0.0, 1.0);
  r->duration_s = duration_s;
  r->finite_fraction = finite_fraction;
  r->noise_rms_db = noise_rms_db;
  r->conservative_noise_rms_db = conservative_rms_db;
  r->noise_peak_db = noise_peak_db;
  r->crest_factor_db = crest_factor_db;
  r->clipped_fraction = clipped_fraction;
  r->zero_fraction = zero_fraction;
  r->rms_spread_db = rms_spread_db;
  r->octave_stability_db = octave_stability_db;
  r->spectral_flux_db = spectral_flux_db;
  r->vad_contamination_ratio = vad_ratio;
  r->vad_contamination_p90 = vad_p90;
  r->capture_age_s = capture_age_s;
  r->in_capture_level_delta_db = level_delta_db;
  r->spectral_shape_distance_db = shape_distance_db;
  r->in_capture_noise_frame_count = quiet_count;
  r->noise_frames = Fn;
  r->speech_frames = Fs;
  r->n_bands = NB;
  r->has_in_capture_spectrum = selected;

  free(w); free(tw); free(buf); free(freqs); free(grid); free(nsum); free(ssum); free(npow); free(spow); free(nrms); free(srms);
  free(npsd); free(bandp); free(explicit_db); free(in_capture_db); free(list);
  return 0;
}
