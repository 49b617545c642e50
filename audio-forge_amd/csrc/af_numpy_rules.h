/* af_numpy_rules.h -- the NumPy rules that the host halves of the analyses share (af_api_spectrum.cpp,
 * af_api_noise_reference.cpp, af_speech_features_math.h), each restated once in f64: np.percentile's linear method, np.median
 * of sorted values, np.interp with held ends, and _interpolate_vad_probabilities (spectrum.py:172-197) on top of it.  Plain C:
 * tests/ref/speech_features_ref.c reads it too. */
#ifndef AF_NUMPY_RULES_H
#define AF_NUMPY_RULES_H
#include <math.h>
#include <stdint.h>

/* np.percentile, method "linear", with its two-sided lerp, over values already sorted */
static inline double af_percentile_sorted(const double *s, int n, double q) {
  const double idx = (q / 100.0) * (double)(n - 1);
  int lo = (int)floor(idx), hi;
  if (lo < 0) lo = 0;
  if (lo > n - 1) lo = n - 1;
  hi = lo + 1 < n - 1 ? lo + 1 : n - 1;
  {
    const double t = idx - (double)lo, a = s[lo], b = s[hi], diff = b - a;
    return t >= 0.5 ? b - diff * (1.0 - t) : a + diff * t;
  }
}

static inline double af_median_sorted(const double *s, int n) { return n % 2 ? s[n / 2] : (s[n / 2 - 1] + s[n / 2]) / 2.0; }

/* np.interp, ends held */
static inline double af_interp(double x, const double *xp, const double *fp, int n) {
  int lo = 0, hi = n - 1;
  if (x < xp[0]) return fp[0];
  if (x >= xp[n - 1]) return fp[n - 1];
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (x >= xp[mid]) lo = mid; else hi = mid;
  }
  return (fp[lo + 1] - fp[lo]) / (xp[lo + 1] - xp[lo]) * (x - xp[lo]) + fp[lo];
}

/* _interpolate_vad_probabilities, spectrum.py:172-197: posteriors of `window` samples each, at the centres of frames of `frame`
 * samples that start every `hop` */
static inline void af_interpolate_vad_probabilities(const double *vad, int64_t n_vad, int64_t window, int frames, int hop, int frame,
                                                    double *xp /* [n_vad] */, double *fp /* [n_vad] */, double *out /* [frames] */) {
  int64_t i;
  int f;
  for (i = 0; i < n_vad; ++i) {
    xp[i] = ((double)i + 0.5) * (double)window;
    fp[i] = vad[i] < 0.0 ? 0.0 : (vad[i] > 1.0 ? 1.0 : vad[i]);
  }
  for (f = 0; f < frames; ++f) out[f] = af_interp((double)((int64_t)f * hop) + (double)frame * 0.5, xp, fp, (int)n_vad);
}

#endif
