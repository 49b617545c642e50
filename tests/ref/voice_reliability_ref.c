/* CPU restatement of the reliability statistics of the voice spectrum measurement (test infrastructure only).
 *
 * Restates the second half of python/mic_eq/analysis/spectrum.py's analyze_voice_spectrum, :647-742, with
 * _robust_median_spectrum (:250-290), _spectral_snr_db (:333-342), _estimate_snr_from_spectrum (:345-365),
 * _estimate_tilt_db_per_octave (:368-378), _coarse_phonetic_coverage (:381-408), _effective_block_count (:411-424) and
 * _measurement_reliability (:427-495), one stream per call.  Its input is what tests/voice_spectrum_oracle.py's analyze returns:
 * the smoothed rows of the voiced windows, their frame starts and the noise reference.
 *
 * Sums run in the order of csrc/af_spectrum_stats.hip: 64 lane-strided partials and an xor tree per row; per stream 256
 * thread-strided partials, an xor tree per wave and the four waves in order.  Medians select, so a sort gives the kernels'
 * values.  The O(windows) parts and the scalars follow csrc/af_api_spectrum.cpp with NumPy's linear percentile and median.
 *
 * Build with -ffp-contract=off and without fast-math (tests/voice_reliability_oracle.py does). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define BLOCK_FRAMES 3            /* UNCERTAINTY_BLOCK_FRAMES, spectrum.py:28 */
#define UNCERTAINTY_SCALE_DB 2.5  /* :29 */
#define TARGET_BLOCKS 12.0        /* PHONETIC_COVERAGE_TARGET_BLOCKS, :30 */
#define BANDS 5
#define LEVEL_FIELDS (2 + BANDS)
#define THREADS 256

typedef struct vrr_row {
  double snr_db, spectral_tilt_db_per_octave, residual_confidence, measurement_coverage, outlier_rejection_ratio;
  double phonetic_coverage, effective_measurement_blocks;
  int32_t voiced, independent, blocks, inliers, used_closest_windows, reserved;
} vrr_row;

static int cmp_double(const void *a, const void *b) {
  const double x = *(const double *)a, y = *(const double *)b;
  return (x > y) - (x < y);
}

static double median_of(double *v, int n) { /* np.median; sorts v */
  qsort(v, (size_t)n, sizeof(double), cmp_double);
  return n % 2 ? v[n / 2] : (v[n / 2 - 1] + v[n / 2]) / 2.0;
}

static double percentile_sorted(const double *s, int n, double q) { /* np.percentile, method "linear" */
  const double idx = (q / 100.0) * (double)(n - 1);
  int lo = (int)floor(idx);
  if (lo < 0) lo = 0;
  if (lo > n - 1) lo = n - 1;
  const int hi = lo + 1 > n - 1 ? n - 1 : lo + 1;
  const double t = idx - (double)lo, a = s[lo], b = s[hi], diff = b - a;
  double r = a + diff * t;
  if (t >= 0.5) r = b - diff * (1.0 - t);
  return r;
}

static double clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

static double xor_tree(double *a /* [64] */) {
  double t[64];
  for (int off = 32; off >= 1; off >>= 1) {
    for (int l = 0; l < 64; ++l) t[l] = a[l] + a[l ^ off];
    memcpy(a, t, sizeof t);
  }
  return a[0];
}

/* the bin ranges of csrc/af_spectrum_host.hpp's vs_make_band_table */
static void band_table(int fs, int N, int *v0, int *v1, int *first, int *last) {
  static const double edges[BANDS + 1] = {100.0, 350.0, 1000.0, 2500.0, 4500.0, 8000.0};
  const int K = N / 2 + 1;
  const double d = 1.0 / (double)fs, val = 1.0 / ((double)N * d);
  *v0 = 0; *v1 = -1;
  for (int k = 0, seen = 0; k < K; ++k) {
    const double f = (double)k * val;
    if (f >= 100.0 && f <= 8000.0) { if (!seen) { *v0 = k; seen = 1; } *v1 = k; }
  }
  if (*v1 < *v0) { *v0 = 0; *v1 = K - 1; }
  for (int b = 0; b < BANDS; ++b) {
    first[b] = 0; last[b] = -1;
    for (int k = 0, seen = 0; k < K; ++k) {
      const double f = (double)k * val;
      if (f >= edges[b] && f < edges[b + 1]) { if (!seen) { first[b] = k; seen = 1; } last[b] = k; }
    }
  }
}

/* np.median of v[0 .. n) with `minus` taken off the one or two selected values */
static double median_minus(const double *v, int n, double minus, double *scratch) {
  memcpy(scratch, v, sizeof(double) * (size_t)n);
  qsort(scratch, (size_t)n, sizeof(double), cmp_double);
  const double a = scratch[(n - 1) / 2], b = scratch[n / 2];
  return (n & 1) ? a - minus : ((a - minus) + (b - minus)) / 2.0;
}

/* per (bin) the median over rows list[0 .. n) of S[row][k] - levels[row][which] (+ add) */
static void offset_median(const double *S, int K, const int *list, int n, const double *levels, int which, int with_add, double add,
                          double *out) {
  double *col = (double *)malloc(sizeof(double) * (size_t)n);
  for (int k = 0; k < K; ++k) {
    for (int i = 0; i < n; ++i) col[i] = S[(size_t)list[i] * K + k] - levels[(size_t)list[i] * LEVEL_FIELDS + which];
    double v = median_of(col, n);
    if (with_add) v = v + add;
    out[k] = v;
  }
  free(col);
}

static void spectral_snr(const double *speech, const double *noise, int K, double *out) { /* :333-342 */
  for (int k = 0; k < K; ++k) {
    const double total = pow(10.0, speech[k] / 10.0);
    double np_ = pow(10.0, noise[k] / 10.0);
    if (np_ < 1e-18) np_ = 1e-18;
    double sig = total - np_;
    if (sig < np_ * 1e-6) sig = np_ * 1e-6;
    out[k] = 10.0 * log10(sig / np_);
  }
}

double vrr_estimate_snr(const double *spectrum, const double *noise, int fs, int N) { /* :345-365 */
  if (!noise) return 0.0;
  const int K = N / 2 + 1;
  const double d = 1.0 / (double)fs, val = 1.0 / ((double)N * d);
  int any = 0;
  for (int k = 0; k < K; ++k) any = any || ((double)k * val >= 80.0 && (double)k * val <= 8000.0);
  double noise_sum = 0.0, signal_sum = 0.0;
  for (int k = 0; k < K; ++k) {
    const double f = (double)k * val;
    if (any && !(f >= 80.0 && f <= 8000.0)) continue;
    const double total = pow(10.0, spectrum[k] / 10.0), np_ = pow(10.0, noise[k] / 10.0);
    noise_sum += np_;
    signal_sum += total - np_;
  }
  if (noise_sum < 1e-18) noise_sum = 1e-18;
  if (signal_sum < noise_sum * 1e-6) signal_sum = noise_sum * 1e-6;
  return 10.0 * log10(signal_sum / noise_sum);
}

double vrr_estimate_tilt(const double *spectrum, int fs, int N) { /* :368-378 */
  const int K = N / 2 + 1;
  const double d = 1.0 / (double)fs, val = 1.0 / ((double)N * d);
  double *x = (double *)malloc(sizeof(double) * (size_t)K), *y = (double *)malloc(sizeof(double) * (size_t)K);
  int n = 0;
  for (int k = 0; k < K; ++k) {
    const double f = (double)k * val;
    if (f >= 100.0 && f <= 8000.0) { x[n] = log2(f); y[n] = spectrum[k]; ++n; }
  }
  double out = 0.0;
  if (n >= 2) {
    double mx = 0.0, my = 0.0, denom = 0.0, dot = 0.0;
    for (int i = 0; i < n; ++i) { mx += x[i]; my += y[i]; }
    mx /= (double)n;
    my /= (double)n;
    for (int i = 0; i < n; ++i) { x[i] -= mx; denom += x[i] * x[i]; }
    if (denom > 0.0) {
      for (int i = 0; i < n; ++i) dot += x[i] * (y[i] - my);
      out = dot / denom;
    }
  }
  free(x); free(y);
  return out;
}

/* One stream on the main branch.  smooth: [V][K] smoothed rows of the voiced windows in frame order; starts: [V] their first
 * samples; noise: null, or the noise reference [K].  Every output pointer may be null: median / repeat / uncertainty / snr [K]
 * (snr NaN without a noise reference), distance / inlier [V], levels [V][7], block_rows [V][K] (the first row->blocks rows are
 * written), stats [4] (lag-one dot product, the two squared norms, effective blocks).  Returns 0, or -1 when V < 3. */
int vrr_analyze(const double *smooth, int V, const int64_t *starts, const double *noise, int fs, int N, vrr_row *row, double *median,
                double *repeat, double *uncertainty, double *snr, double *distance, uint8_t *inlier, double *levels_out,
                double *block_rows_out, double *stats_out) {
  if (V < 3) return -1;
  const int K = N / 2 + 1;
  int v0, v1, first[BANDS], last[BANDS];
  band_table(fs, N, &v0, &v1, first, last);
  const int nb = v1 - v0 + 1;
  double *levels = (double *)malloc(sizeof(double) * (size_t)V * LEVEL_FIELDS), *scratch = (double *)malloc(sizeof(double) * (size_t)(K > V ? K : V));
  double part[64];

  /* vs_row_levels_kernel */
  for (int r = 0; r < V; ++r) {
    const double *v = smooth + (size_t)r * K + v0;
    for (int l = 0; l < 64; ++l) {
      double a = 0.0;
      for (int i = l; i < nb; i += 64) a += v[i];
      part[l] = a;
    }
    const double mean = xor_tree(part) / (double)nb;
    double *out = levels + (size_t)r * LEVEL_FIELDS;
    out[0] = mean;
    out[1] = median_minus(v, nb, 0.0, scratch);
    for (int b = 0; b < BANDS; ++b) {
      const int n = last[b] - first[b] + 1;
      out[2 + b] = n > 0 ? median_minus(smooth + (size_t)r * K + first[b], n, mean, scratch) : NAN;
    }
  }

  /* the host's lists: independent windows (:446-454), blocks (:456-463) */
  int *independent = (int *)malloc(sizeof(int) * (size_t)V), *list = (int *)malloc(sizeof(int) * (size_t)V), ni = 0;
  int64_t next_start = -1;
  for (int j = 0; j < V; ++j)
    if (starts[j] >= next_start) { independent[ni++] = j; next_start = starts[j] + N; }
  double *blocks = (double *)malloc(sizeof(double) * (size_t)V * K), *centre = (double *)malloc(sizeof(double) * (size_t)K);
  int nblk = 0;
  for (int b = 0; b < ni / BLOCK_FRAMES; ++b)
    offset_median(smooth, K, independent + b * BLOCK_FRAMES, BLOCK_FRAMES, levels, 0, 0, 0.0, blocks + (size_t)(nblk++) * K);
  if (nblk == 0 && ni > 0) offset_median(smooth, K, independent, ni, levels, 0, 0, 0.0, blocks + (size_t)(nblk++) * K);
  for (int j = 0; j < V; ++j) list[j] = j;
  offset_median(smooth, K, list, V, levels, 1, 0, 0.0, centre); /* :270 */

  /* vs_shape_distance_kernel */
  double *dist = (double *)malloc(sizeof(double) * (size_t)V);
  for (int r = 0; r < V; ++r) {
    const double *s = smooth + (size_t)r * K, level = levels[(size_t)r * LEVEL_FIELDS + 1];
    for (int l = 0; l < 64; ++l) {
      double a = 0.0;
      for (int i = v0 + l; i <= v1; i += 64) {
        const double d = (s[i] - level) - centre[i];
        a += d * d;
      }
      part[l] = a;
    }
    dist[r] = sqrt(xor_tree(part) / (double)nb);
  }

  /* vs_block_stats_kernel */
  double *unc = (double *)malloc(sizeof(double) * (size_t)K), *rel = (double *)malloc(sizeof(double) * (size_t)K);
  double stats[4] = {0.0, 0.0, 0.0, (double)nblk};
  if (nblk < 2) {
    for (int k = 0; k < K; ++k) { unc[k] = INFINITY; rel[k] = 0.0; }
  } else {
    double pd[THREADS], pl[THREADS], pr[THREADS];
    for (int t = 0; t < THREADS; ++t) {
      double dot = 0.0, nl = 0.0, nr = 0.0;
      for (int k = t; k < K; k += THREADS) {
        for (int j = 0; j < nblk; ++j) scratch[j] = blocks[(size_t)j * K + k];
        const double c = median_of(scratch, nblk);
        for (int j = 0; j + 1 < nblk; ++j) {
          const double l = blocks[(size_t)j * K + k] - c, r = blocks[(size_t)(j + 1) * K + k] - c;
          dot += l * r;
          nl += l * l;
          nr += r * r;
        }
        for (int j = 0; j < nblk; ++j) scratch[j] = fabs(blocks[(size_t)j * K + k] - c);
        unc[k] = 1.4826 * median_of(scratch, nblk);
      }
      pd[t] = dot; pl[t] = nl; pr[t] = nr;
    }
    double dot = 0.0, nl = 0.0, nr = 0.0;
    for (int w = 0; w < THREADS / 64; ++w) {
      const double a = xor_tree(pd + 64 * w), b = xor_tree(pl + 64 * w), c = xor_tree(pr + 64 * w);
      dot = w ? dot + a : a;
      nl = w ? nl + b : b;
      nr = w ? nr + c : c;
    }
    const double denominator = sqrt(nl) * sqrt(nr);
    double lag = 0.95;
    if (!(denominator <= 1e-12)) lag = clip(dot / denominator, 0.0, 0.95);
    const double effective = clip((double)nblk * (1.0 - lag) / (1.0 + lag), 1.0, (double)nblk);
    const double root = sqrt(effective > 1.0 ? effective : 1.0);
    for (int k = 0; k < K; ++k) {
      const double u = (1.253 * unc[k] + 0.35) / root, q = u / UNCERTAINTY_SCALE_DB;
      unc[k] = u;
      rel[k] = clip(exp(-(q * q)), 0.0, 1.0);
    }
    stats[0] = dot; stats[1] = nl; stats[2] = nr; stats[3] = effective;
  }

  /* the inliers, :276-289 */
  memcpy(scratch, dist, sizeof(double) * (size_t)V);
  const double mid = median_of(scratch, V);
  for (int j = 0; j < V; ++j) scratch[j] = fabs(dist[j] - mid);
  const double mad = median_of(scratch, V), cutoff = mid + 4.0 * (mad > 0.25 ? mad : 0.25);
  uint8_t *in = (uint8_t *)malloc((size_t)V);
  int count = 0, closest = 0;
  for (int j = 0; j < V; ++j) count += in[j] = dist[j] <= cutoff;
  int minimum = (int)ceil((double)V * 0.50);
  if (minimum < 3) minimum = 3;
  if (count < minimum) { /* the closest windows: a stable selection by distance */
    memset(in, 0, (size_t)V);
    for (int pick = 0; pick < minimum && pick < V; ++pick) {
      int best = -1;
      for (int j = 0; j < V; ++j)
        if (!in[j] && (best < 0 || dist[j] < dist[best])) best = j;
      in[best] = 1;
    }
    count = minimum < V ? minimum : V;
    closest = 1;
  }
  int n_in = 0;
  for (int j = 0; j < V; ++j)
    if (in[j]) { scratch[n_in] = levels[(size_t)j * LEVEL_FIELDS + 1]; list[n_in] = j; ++n_in; }
  const double robust_level = median_of(scratch, n_in);
  double *med = (double *)malloc(sizeof(double) * (size_t)K), *sn = (double *)malloc(sizeof(double) * (size_t)K);
  offset_median(smooth, K, list, n_in, levels, 1, 1, robust_level, med); /* :287-290 */

  /* the scalars, :673-721 */
  double diversity = 0.0;
  int scores = 0;
  static const double targets[BANDS] = {3.0, 4.0, 5.0, 6.0, 7.0};
  for (int b = 0; b < BANDS; ++b) {
    if (last[b] < first[b]) continue;
    for (int i = 0; i < ni; ++i) scratch[i] = levels[(size_t)independent[i] * LEVEL_FIELDS + 2 + b];
    qsort(scratch, (size_t)ni, sizeof(double), cmp_double);
    const double spread = percentile_sorted(scratch, ni, 90.0) - percentile_sorted(scratch, ni, 10.0);
    diversity += clip(spread / targets[b], 0.0, 1.0);
    ++scores;
  }
  diversity = scores ? diversity / (double)scores : 0.0;
  const double duration = clip(stats[3] / TARGET_BLOCKS, 0.0, 1.0);
  const double phonetic = sqrt(diversity * duration);
  const double inlier_ratio = (double)count / (double)(V > 1 ? V : 1);
  if (noise) spectral_snr(med, noise, K, sn);
  else for (int k = 0; k < K; ++k) sn[k] = NAN;
  const double snr_db = vrr_estimate_snr(med, noise, fs, N);
  memcpy(scratch, rel + v0, sizeof(double) * (size_t)nb);
  const double score = median_of(scratch, nb);
  const double coverage = clip(0.45 * inlier_ratio + 0.35 * phonetic + 0.20 * duration, 0.0, 1.0);
  double confidence;
  if (!noise) confidence = clip(0.5625 * score + 0.4375 * phonetic, 0.0, 0.70);
  else confidence = clip(0.45 * score + 0.35 * phonetic + 0.20 * clip((snr_db - 3.0) / 15.0, 0.0, 1.0), 0.0, 1.0);
  if (row) {
    row->snr_db = snr_db;
    row->spectral_tilt_db_per_octave = vrr_estimate_tilt(med, fs, N);
    row->residual_confidence = clip(confidence * (0.75 + 0.25 * coverage), 0.0, 1.0);
    row->measurement_coverage = coverage;
    row->outlier_rejection_ratio = 1.0 - inlier_ratio;
    row->phonetic_coverage = phonetic;
    row->effective_measurement_blocks = stats[3];
    row->voiced = V;
    row->independent = ni;
    row->blocks = nblk;
    row->inliers = count;
    row->used_closest_windows = closest;
    row->reserved = 0;
  }
  const size_t kb = sizeof(double) * (size_t)K;
  if (median) memcpy(median, med, kb);
  if (repeat) memcpy(repeat, rel, kb);
  if (uncertainty) memcpy(uncertainty, unc, kb);
  if (snr) memcpy(snr, sn, kb);
  if (distance) memcpy(distance, dist, sizeof(double) * (size_t)V);
  if (inlier) memcpy(inlier, in, (size_t)V);
  if (levels_out) memcpy(levels_out, levels, sizeof(double) * (size_t)V * LEVEL_FIELDS);
  if (block_rows_out) memcpy(block_rows_out, blocks, kb * (size_t)nblk);
  if (stats_out) memcpy(stats_out, stats, sizeof stats);
  free(levels); free(scratch); free(independent); free(list); free(blocks); free(centre); free(dist); free(unc); free(rel); free(in);
  free(med); free(sn);
  return 0;
}
