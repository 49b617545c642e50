/* CPU restatement of the voice spectrum measurement (test infrastructure only).
 *
 * Restates python/mic_eq/analysis/spectrum.py:69-343 (_select_voiced_samples, compute_voice_spectrum, _frame_rms_db,
 * _interpolate_vad_probabilities, _voiced_frame_mask, _window_spectrum_db, _median_frame_spectrum_db,
 * _audio_reference_spectrum_db, _spectral_snr_db), :519-645 (analyze_voice_spectrum up to its single-spectrum fallback) and
 * :839-967 (get_octave_frequencies, smooth_spectrum_octave, smooth_spectrum_perceptual "balanced"), one stream per call.
 *
 * Where the reference calls NumPy / SciPy (np.mean, np.fft.rfft, signal.welch) this file uses the arithmetic of
 * csrc/af_spectrum.hip instead, operation for operation: hop-sized chunk sums over 64 strided partials and an xor tree, a
 * radix-2 decimation-in-frequency complex transform of half the frame length with the real-input split behind it, twiddles
 * and the Hamming window from the same f64 formulas the library uploads.  tests/test_voice_spectrum_ref.py holds it to the
 * reference's recorded outputs within a measured tolerance; the GPU tests then hold the kernels to it bit for bit.
 *
 * Build with -ffp-contract=off and without fast-math (tests/voice_spectrum_oracle.py does). */
#define _GNU_SOURCE /* sincos */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define RMS_GATE_DB (-48.0)        /* VOICE_FRAME_RMS_GATE_DB, spectrum.py:17 */
#define FLOOR_PERCENTILE 20.0      /* :18 */
#define PEAK_PERCENTILE 95.0       /* :19 */
#define GATE_FRACTION 0.60         /* :20 */
#define MIN_SPREAD_DB 6.0          /* :21 */
#define MIN_VOICED_RATIO 0.15      /* :22 */
#define MIN_VOICED_FRAMES 3        /* :23 */
#define SILERO_WINDOW 512          /* :24 */
#define SILERO_RATE 16000          /* :25 */
#define VAD_EVIDENCE 0.4           /* analysis/vad.py */
#define VAD_STRONG 0.65
#define PI 3.14159265358979323846

enum { SRC_UNAVAILABLE = 0, SRC_EXPLICIT = 1, SRC_IN_CAPTURE = 2 };

typedef struct vsr_row {
  int32_t frames, voiced;
  double voiced_window_ratio;
  int32_t vad_probability_used;
  double vad_active_window_ratio;
  int32_t noise_reference_source;
  int32_t used_single_spectrum_fallback;
  int32_t welch_segments;
} vsr_row;

/* ---- tables: the formulas of af_spectrum_host.hpp ---- */
static void make_window(int N, double *w, double *sumw2) {
  double s = 0.0;
  for (int i = 0; i < N; ++i) {  /* np.hamming: 0.54 + 0.46 cos(pi n / (N - 1)), n = 1 - N, 3 - N, ... */
    w[i] = 0.54 + 0.46 * cos(PI * (double)(2 * i + 1 - N) / (double)(N - 1));
    s += w[i] * w[i];
  }
  *sumw2 = s;
}

/* signal.welch's window: get_window("hamming", N) is periodic -- the symmetric window of N + 1 points without its last */
static void make_welch_window(int N, double *w, double *sumw2) {
  const double step = (PI - (-PI)) / (double)N;  /* np.linspace(-pi, pi, N + 1) */
  double s = 0.0;
  for (int i = 0; i < N; ++i) {
    w[i] = 0.54 + 0.46 * cos((double)i * step + (-PI));
    s += w[i] * w[i];
  }
  *sumw2 = s;
}

static void make_twiddles(int N, double *tw /* [N/2 + 1][2] */) {
  for (int k = 0; k <= N / 2; ++k) {
    const double a = -2.0 * PI * (double)k / (double)N;
    sincos(a, &tw[2 * k + 1], &tw[2 * k]);  /* one libm entry in both builds: a compiler may or may not merge cos() and sin() */
  }
}

void vsr_freqs(int fs, int N, double *f) {  /* np.fft.rfftfreq(N, 1 / fs) */
  const double d = 1.0 / (double)fs;
  const double val = 1.0 / ((double)N * d);
  for (int k = 0; k <= N / 2; ++k) f[k] = (double)k * val;
}

/* get_octave_frequencies(fraction), limits (20, 20000), ref 1000: spectrum.py:839-889.  Returns the band count. */
int vsr_octave_bands(int b, double *centre, double *lower, double *upper) {
  const double G = pow(10.0, 0.3);
  const int x_min = (int)floor((double)b * log10(20.0 / 1000.0) / log10(G));
  const int x_max = (int)ceil((double)b * log10(20000.0 / 1000.0) / log10(G));
  int n = 0;
  for (int x = x_min; x <= x_max; ++x) {
    const double fm = (b % 2 == 1) ? 1000.0 * pow(G, (double)x / (double)b)
                                   : 1000.0 * pow(G, (double)(2 * x + 1) / (double)(2 * b));
    if (20.0 <= fm && fm <= 20000.0) {
      const double h = pow(G, 1.0 / (double)(2 * b));
      centre[n] = fm;
      lower[n] = fm / h;
      upper[n] = fm * h;
      ++n;
    }
  }
  return n;
}

/* ---- the kernels' arithmetic ---- */
/* one hop-sized chunk: 64 strided partial sums, then the xor tree (every lane ends with the same value) */
static void chunk_sums(const float *x, int hop, double *sx, double *sxx) {
  double a[64], q[64], ta[64], tq[64];
  for (int l = 0; l < 64; ++l) {
    double s = 0.0, ss = 0.0;
    for (int i = l; i < hop; i += 64) {
      const double v = (double)x[i];
      s += v;
      ss += v * v;
    }
    a[l] = s;
    q[l] = ss;
  }
  for (int off = 32; off >= 1; off >>= 1) {
    for (int l = 0; l < 64; ++l) { ta[l] = a[l] + a[l ^ off]; tq[l] = q[l] + q[l ^ off]; }
    memcpy(a, ta, sizeof a);
    memcpy(q, tq, sizeof q);
  }
  *sx = a[0];
  *sxx = q[0];
}

static unsigned bitrev(unsigned v, int bits) {
  unsigned r = 0;
  for (int i = 0; i < bits; ++i) { r = (r << 1) | (v & 1u); v >>= 1; }
  return r;
}

/* |rfft((x - mean) * w)|^2 of the frame made of two chunks, bins 0 .. N/2 */
static void segment_power(const float *ca, const float *cb, double sxa, double sxb, int N, const double *w, const double *tw,
                          double *buf /* [N] scratch */, double *p) {
  const int M = N / 2;
  const double mean = (sxa + sxb) / (double)N;
  for (int i = 0; i < N; ++i) {
    const float s = i < M ? ca[i] : cb[i - M];
    buf[i] = ((double)s - mean) * w[i];  /* buf[2m], buf[2m + 1] = re, im of z[m] */
  }
  int bits = 0;
  while ((1 << bits) < M) ++bits;
  for (int half = M / 2; half >= 1; half >>= 1) {
    const int step = M / (2 * half);
    for (int j = 0; j < M / 2; ++j) {
      const int pos = j % half, i0 = (j / half) * 2 * half + pos, i1 = i0 + half;
      const double ar = buf[2 * i0], ai = buf[2 * i0 + 1], br = buf[2 * i1], bi = buf[2 * i1 + 1];
      const double dr = ar - br, di = ai - bi;
      const double tr = tw[2 * (2 * pos * step)], ti = tw[2 * (2 * pos * step) + 1];  /* exp(-2 pi i pos step / M) */
      buf[2 * i0] = ar + br;
      buf[2 * i0 + 1] = ai + bi;
      buf[2 * i1] = dr * tr - di * ti;
      buf[2 * i1 + 1] = dr * ti + di * tr;
    }
  }
  for (int k = 0; k <= M; ++k) {
    const unsigned ia = bitrev((unsigned)(k % M), bits), ib = bitrev((unsigned)((M - k) % M), bits);
    const double ar = buf[2 * ia], ai = buf[2 * ia + 1], br = buf[2 * ib], bi = buf[2 * ib + 1];
    const double er = 0.5 * (ar + br), ei = 0.5 * (ai - bi);
    const double orr = 0.5 * (ai + bi), oi = -0.5 * (ar - br);
    const double tr = tw[2 * k], ti = tw[2 * k + 1];
    const double xr = er + (orr * tr - oi * ti), xi = ei + (orr * ti + oi * tr);
    p[k] = xr * xr + xi * xi;
  }
}

/* ---- NumPy's host-side pieces ---- */
static int cmp_double(const void *a, const void *b) {
  const double x = *(const double *)a, y = *(const double *)b;
  return (x > y) - (x < y);
}

static double percentile_sorted(const double *s, int n, double q) {  /* np.percentile, method "linear" */
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

static double median_of(double *v, int n) {  /* np.median; sorts v */
  qsort(v, (size_t)n, sizeof(double), cmp_double);
  return n % 2 ? v[n / 2] : (v[n / 2 - 1] + v[n / 2]) / 2.0;
}

static double clip01(double v) { return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); }

static double interp1(double x, const double *xp, const double *fp, int n) {  /* np.interp, ends held */
  if (x < xp[0]) return fp[0];
  if (x >= xp[n - 1]) return fp[n - 1];
  int lo = 0, hi = n - 1;  /* xp[lo] <= x < xp[hi] */
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (x >= xp[mid]) lo = mid; else hi = mid;
  }
  const double slope = (fp[lo + 1] - fp[lo]) / (xp[lo + 1] - xp[lo]);
  return slope * (x - xp[lo]) + fp[lo];
}

static void spectral_snr(const double *speech, const double *noise, int K, double *out) {  /* spectrum.py:333-342 */
  for (int k = 0; k < K; ++k) {
    const double total = pow(10.0, speech[k] / 10.0);
    double np_ = pow(10.0, noise[k] / 10.0);
    if (np_ < 1e-18) np_ = 1e-18;
    double sig = total - np_;
    if (sig < np_ * 1e-6) sig = np_ * 1e-6;
    out[k] = 10.0 * log10(sig / np_);
  }
}

/* column medians of rows[n][K] (dB): np.median(axis=0) */
static void column_median(const double *rows, int n, int K, double *out) {
  double *col = (double *)malloc(sizeof(double) * (size_t)(n > 0 ? n : 1));
  for (int k = 0; k < K; ++k) {
    for (int i = 0; i < n; ++i) col[i] = rows[(size_t)i * K + k];
    out[k] = median_of(col, n);
  }
  free(col);
}

/* smooth_spectrum_perceptual(freqs, db, "balanced"): spectrum.py:892-967 */
void vsr_smooth(const double *db, int fs, int N, double *out) {
  const int K = N / 2 + 1;
  static const int fractions[3] = {3, 6, 12};  /* wide, medium, fine (the 1/2-octave pass is not read by "balanced") */
  double *f = (double *)malloc(sizeof(double) * K), *pw = (double *)malloc(sizeof(double) * K);
  double *sm[3];
  vsr_freqs(fs, N, f);
  for (int k = 0; k < K; ++k) pw[k] = pow(10.0, db[k] / 10.0);
  for (int p = 0; p < 3; ++p) {
    double c[256], lo[256], up[256], xc[256], y[256];
    const int nb = vsr_octave_bands(fractions[p], c, lo, up);
    int nv = 0;
    for (int b = 0; b < nb; ++b) {
      int first = -1, last = -1;
      for (int k = 0; k < K; ++k)
        if (f[k] >= lo[b] && f[k] <= up[b]) { if (first < 0) first = k; last = k; }
      if (first < 0) continue;
      double s = 0.0;
      for (int k = first; k <= last; ++k) s += pw[k];
      xc[nv] = c[b];
      y[nv] = 10.0 * log10(s / (double)(last - first + 1));
      ++nv;
    }
    sm[p] = (double *)malloc(sizeof(double) * K);
    for (int k = 0; k < K; ++k) sm[p][k] = nv > 1 ? interp1(f[k], xc, y, nv) : db[k];
  }
  for (int k = 0; k < K; ++k) {
    const int p = f[k] < 180.0 ? 0 : (f[k] < 3500.0 ? 1 : (f[k] <= 9000.0 ? 2 : 0));
    out[k] = sm[p][k];
  }
  for (int p = 0; p < 3; ++p) free(sm[p]);
  free(f);
  free(pw);
}

/* One stream.  Every output pointer may be null.  win_*: [voiced][K] rows of the voiced frames in frame order.
 * gates: [4] the _select_voiced_samples gate, the _voiced_frame_mask gate, the supported-energy gate, voiced - unvoiced level
 * (NaN where not evaluated).  Returns 0, or -1 when n < N. */
int vsr_analyze(const float *audio, int64_t n, const double *vad, int64_t n_vad, const float *noise, int64_t n_noise, int fs, int N,
                vsr_row *row, double *frame_power, double *frame_rms_db, uint8_t *voiced_mask, double *speech_db,
                double *noise_db, double *snr_db, double *welch_db, double *welch_sum, double *win_linear, double *win_db,
                double *win_smooth, double *gates) {
  if (n < N) return -1;
  const int hop = N / 2, K = N / 2 + 1;
  const int F = (int)((n - N) / hop) + 1, C = F + 1;
  double *w = (double *)malloc(sizeof(double) * N), *tw = (double *)malloc(sizeof(double) * 2 * (N / 2 + 1));
  double *buf = (double *)malloc(sizeof(double) * N), *p = (double *)malloc(sizeof(double) * K);
  double *sx = (double *)malloc(sizeof(double) * C), *sxx = (double *)malloc(sizeof(double) * C);
  double *rms = (double *)malloc(sizeof(double) * F), *sorted = (double *)malloc(sizeof(double) * F);
  uint8_t *mask = (uint8_t *)malloc((size_t)F);
  double *ww = (double *)malloc(sizeof(double) * N);
  double sumw2, welch_sumw2;
  make_window(N, w, &sumw2);
  make_welch_window(N, ww, &welch_sumw2);
  make_twiddles(N, tw);
  const double nan_ = NAN;
  if (gates) gates[0] = gates[1] = gates[2] = gates[3] = nan_;

  for (int c = 0; c < C; ++c) chunk_sums(audio + (size_t)c * hop, hop, &sx[c], &sxx[c]);
  for (int f = 0; f < F; ++f) {
    const double power = (sxx[f] + sxx[f + 1]) / (double)N;
    if (frame_power) frame_power[f] = power;
    rms[f] = 10.0 * log10(power + 1e-12);
    sorted[f] = rms[f];
  }
  qsort(sorted, (size_t)F, sizeof(double), cmp_double);
  const double floor_db = percentile_sorted(sorted, F, FLOOR_PERCENTILE), peak_db = percentile_sorted(sorted, F, PEAK_PERCENTILE);
  const double spread = peak_db - floor_db, wide = spread > MIN_SPREAD_DB ? spread : MIN_SPREAD_DB;

  /* _voiced_frame_mask, :200-247 */
  double gate = floor_db + GATE_FRACTION * wide;
  if (gate < RMS_GATE_DB) gate = RMS_GATE_DB;
  if (gates && !(spread < MIN_SPREAD_DB)) gates[1] = gate;
  for (int f = 0; f < F; ++f) mask[f] = spread < MIN_SPREAD_DB ? 1 : (rms[f] >= gate);
  int vad_used = 0;
  double vad_active = 0.0;
  if (vad && n_vad > 0 && fs > 0) {  /* _interpolate_vad_probabilities, :172-197 */
    double *xp = (double *)malloc(sizeof(double) * (size_t)n_vad), *fp = (double *)malloc(sizeof(double) * (size_t)n_vad);
    uint8_t *comb = (uint8_t *)malloc((size_t)F);
    int64_t win = (int64_t)ceil((double)fs * (double)SILERO_WINDOW / (double)SILERO_RATE);
    if (win < 1) win = 1;
    for (int64_t i = 0; i < n_vad; ++i) { xp[i] = ((double)i + 0.5) * (double)win; fp[i] = clip01(vad[i]); }
    double support = floor_db + 0.25 * wide;
    if (support < RMS_GATE_DB) support = RMS_GATE_DB;
    if (gates) gates[2] = support;
    int count = 0, active = 0;
    for (int f = 0; f < F; ++f) {
      const double centre = (double)((int64_t)f * hop) + (double)N * 0.5;
      const double post = interp1(centre, xp, fp, (int)n_vad);
      active += post >= VAD_EVIDENCE;
      comb[f] = (post >= VAD_EVIDENCE && rms[f] >= support) || post >= VAD_STRONG;
      count += comb[f];
    }
    if (count >= MIN_VOICED_FRAMES) memcpy(mask, comb, (size_t)F);
    vad_used = 1;
    vad_active = (double)active / (double)F;
    free(xp); free(fp); free(comb);
  }
  int voiced = 0;
  for (int f = 0; f < F; ++f) voiced += mask[f];
  const double ratio = (double)voiced / (double)F;

  /* window spectra of every frame the medians need */
  double *rows = (double *)malloc(sizeof(double) * (size_t)F * K);
  for (int f = 0, v = 0; f < F; ++f) {
    segment_power(audio + (size_t)f * hop, audio + (size_t)(f + 1) * hop, sx[f], sx[f + 1], N, w, tw, buf, p);
    for (int k = 0; k < K; ++k) {
      const double psd = p[k] / sumw2;
      rows[(size_t)f * K + k] = 10.0 * log10(psd + 1e-12);
      if (mask[f] && win_linear) win_linear[(size_t)v * K + k] = psd;
    }
    if (mask[f]) {
      if (win_db) memcpy(win_db + (size_t)v * K, rows + (size_t)f * K, sizeof(double) * K);
      if (win_smooth) vsr_smooth(rows + (size_t)f * K, fs, N, win_smooth + (size_t)v * K);
      ++v;
    }
  }
  double *sel = (double *)malloc(sizeof(double) * (size_t)F * K);
  double *speech = (double *)malloc(sizeof(double) * K), *nz = (double *)malloc(sizeof(double) * K);
  int have_speech = 0, source = SRC_UNAVAILABLE;
  if (voiced > 0) {
    int v = 0;
    for (int f = 0; f < F; ++f)
      if (mask[f]) memcpy(sel + (size_t)(v++) * K, rows + (size_t)f * K, sizeof(double) * K);
    column_median(sel, voiced, K, speech);
    have_speech = 1;
  }
  if (noise && n_noise >= N) {  /* _audio_reference_spectrum_db, :320-330 */
    const int Fn = (int)((n_noise - N) / hop) + 1;
    double *nrows = (double *)malloc(sizeof(double) * (size_t)Fn * K);
    double *nsx = (double *)malloc(sizeof(double) * (Fn + 1)), dummy;
    for (int c = 0; c <= Fn; ++c) chunk_sums(noise + (size_t)c * hop, hop, &nsx[c], &dummy);
    for (int f = 0; f < Fn; ++f) {
      segment_power(noise + (size_t)f * hop, noise + (size_t)(f + 1) * hop, nsx[f], nsx[f + 1], N, w, tw, buf, p);
      for (int k = 0; k < K; ++k) nrows[(size_t)f * K + k] = 10.0 * log10(p[k] / sumw2 + 1e-12);
    }
    column_median(nrows, Fn, K, nz);
    source = SRC_EXPLICIT;
    free(nrows); free(nsx);
  } else if (F - voiced >= MIN_VOICED_FRAMES && voiced > 0) {  /* :578-586 */
    double *lv = (double *)malloc(sizeof(double) * F), *lu = (double *)malloc(sizeof(double) * F);
    int a = 0, b = 0;
    for (int f = 0; f < F; ++f) { if (mask[f]) lv[a++] = rms[f]; else lu[b++] = rms[f]; }
    const double diff = median_of(lv, a) - median_of(lu, b);
    if (gates) gates[3] = diff;
    if (diff >= 3.0) {
      int u = 0;
      for (int f = 0; f < F; ++f)
        if (!mask[f]) memcpy(sel + (size_t)(u++) * K, rows + (size_t)f * K, sizeof(double) * K);
      column_median(sel, u, K, nz);
      source = SRC_IN_CAPTURE;
    }
    free(lv); free(lu);
  }
  const int have_noise = source != SRC_UNAVAILABLE && have_speech;
  for (int k = 0; k < K; ++k) {
    if (speech_db) speech_db[k] = have_speech ? speech[k] : nan_;
    if (noise_db) noise_db[k] = have_noise ? nz[k] : nan_;
    if (snr_db) snr_db[k] = nan_;
  }
  if (have_noise && snr_db) spectral_snr(speech, nz, K, snr_db);

  /* compute_voice_spectrum, :69-164: the chunks _select_voiced_samples keeps, then Welch over them */
  int *chunks = (int *)malloc(sizeof(int) * C), nc = 0;
  {
    double g2 = floor_db + GATE_FRACTION * spread;
    if (g2 < RMS_GATE_DB) g2 = RMS_GATE_DB;
    int cnt = 0, whole = spread < MIN_SPREAD_DB;
    if (!whole) {
      if (gates) gates[0] = g2;
      for (int f = 0; f < F; ++f) cnt += rms[f] >= g2;
      if (cnt < MIN_VOICED_FRAMES || (double)cnt / (double)F < MIN_VOICED_RATIO) whole = 1;
    }
    for (int c = 0; c < C; ++c) {
      const int keep = whole || (c < F && rms[c] >= g2) || (c > 0 && rms[c - 1] >= g2);
      if (keep) chunks[nc++] = c;
    }
  }
  double *acc = (double *)calloc((size_t)K, sizeof(double));
  const int nseg = nc - 1;
  for (int j = 0; j < nseg; ++j) {
    const int a = chunks[j], b = chunks[j + 1];
    segment_power(audio + (size_t)a * hop, audio + (size_t)b * hop, sx[a], sx[b], N, ww, tw, buf, p);
    for (int k = 0; k < K; ++k) acc[k] = j == 0 ? p[k] : acc[k] + p[k];
  }
  const double scale = 1.0 / ((double)fs * welch_sumw2);
  for (int k = 0; k < K; ++k) {
    double v = acc[k] * scale;
    if (k > 0 && k < K - 1) v = v * 2.0;
    v = v / (double)nseg;
    if (welch_sum) welch_sum[k] = acc[k];
    if (welch_db) welch_db[k] = 10.0 * log10(v + 1e-12);
  }

  const int fallback = voiced < MIN_VOICED_FRAMES || ratio < MIN_VOICED_RATIO;
  if (row) {
    row->frames = F;
    row->voiced = voiced;
    row->voiced_window_ratio = fallback ? (ratio > 1.0 / (double)F ? ratio : 1.0 / (double)F) : ratio;
    row->vad_probability_used = vad_used;
    row->vad_active_window_ratio = vad_active;
    row->noise_reference_source = source;
    row->used_single_spectrum_fallback = fallback;
    row->welch_segments = nseg;
  }
  for (int f = 0; f < F; ++f) {
    if (frame_rms_db) frame_rms_db[f] = rms[f];
    if (voiced_mask) voiced_mask[f] = mask[f];
  }
  free(w); free(ww); free(tw); free(buf); free(p); free(sx); free(sxx); free(rms); free(sorted); free(mask); free(rows); free(sel);
  free(speech); free(nz); free(chunks); free(acc);
  return 0;
}
