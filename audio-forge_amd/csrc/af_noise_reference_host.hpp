// af_noise_reference_host.hpp -- what the host side and the kernels of the room-noise reference analysis
// (af_noise_reference.hip) share: the constants of python/mic_eq/analysis/noise_reference.py, the tables the host computes in
// f64 and uploads (Hann window, twiddles, factor list, octave-band bin ranges), the work records and the launchers.
//
// Frame sizes.  The frame is N = max(512, round(0.2 fs)) samples at hop N / 2 (:119-122).  The transform takes N that is even,
// whose half M = N / 2 has no prime factor above 7, and whose M complex f64 points fit the 160 KB of LDS a workgroup can have
// (M <= 10240).  That holds for 8, 12, 16, 22.05, 24, 32, 44.1, 48, 64 and 96 kHz and for every rate up to 2560 Hz
// (N = 512); 88.2 kHz (M = 8820 = 2^2 3^2 5 7^2) fits too, 192 kHz (M = 19200) does not.  Anything else is refused when the
// handle is created.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>

#include <cmath>
#include <cstdint>
#include <vector>

namespace af {

constexpr double kNrMinDurationS = 1.5;         // MIN_NOISE_DURATION_S, noise_reference.py:12
constexpr double kNrQuestionableAgeS = 120.0;   // :13
constexpr double kNrInvalidAgeS = 600.0;        // :14
constexpr double kNrVadContamination = 0.35;    // VAD_NOISE_CONTAMINATION_THRESHOLD, analysis/vad.py
constexpr int kNrBands = 7;                     // OCTAVE_CENTERS_HZ, :15-18: 125 Hz .. 8 kHz
constexpr int kNrMaxFactors = 16;
constexpr int kNrMaxHalf = 10240;               // 16 bytes a point in 160 KB
constexpr int kNrThreads = 256;
constexpr int kNrTileStreams = 64;              // the PSD scratch is sized for at most this many streams

// what nr_sample_stats_kernel leaves per stream, :294-307 (non-finite samples count as 0 everywhere but in `finite`)
struct NrSampleStats { double sum_squares, peak; int64_t finite, clipped, zero; };
// the factors of M = N / 2 in the order the transform takes them
struct NrPlan { int32_t n_factors, factor[kNrMaxFactors]; };
// the octave bands that hold a bin, in centre order: bins first[b] .. last[b]
struct NrBandTable { int32_t n_bands, first[kNrBands], last[kNrBands]; };
// one frame: the one of `source` (0 the noise capture, 1 the voice capture) that starts at chunk `chunk`, into scratch row `row`
struct NrFrameItem { int32_t source, stream, chunk, row; };

inline int nr_frame_size(uint32_t fs) {  // max(512, int(round(fs * 0.20))), :119; Python rounds halves to even
  const double r = std::nearbyint((double)fs * 0.20);
  return r < 512.0 ? 512 : (int)r;
}

// false when M has a prime factor above 7.  Largest radix first: the short strides of the last stages belong to the cheap butterflies.
inline bool nr_make_plan(int M, NrPlan &plan) {
  static const int radices[4] = {7, 5, 3, 2};
  plan = NrPlan{};
  for (int p : radices)
    while (M % p == 0 && plan.n_factors < kNrMaxFactors) { plan.factor[plan.n_factors++] = p; M /= p; }
  return M == 1;
}

inline void nr_make_window(int N, std::vector<double> &w, double *sumw2) {  // np.hanning(N), :131-132
  const double pi = 3.14159265358979323846;
  w.resize((size_t)N);
  double s = 0.0;
  for (int i = 0; i < N; ++i) {  // 0.5 + 0.5 cos(pi n / (N - 1)), n = 1 - N, 3 - N, ...
    w[(size_t)i] = 0.5 + 0.5 * std::cos(pi * (double)(2 * i + 1 - N) / (double)(N - 1));
    s += w[(size_t)i] * w[(size_t)i];
  }
  *sumw2 = s > 1e-18 ? s : 1e-18;
}

inline void nr_make_twiddles(int N, std::vector<double> &tw) {  // exp(-2 pi i k / N), k = 0 .. N - 1, (re, im) pairs
  const double pi = 3.14159265358979323846;
  tw.resize(2 * (size_t)N);
  for (int k = 0; k < N; ++k) {
    const double a = -2.0 * pi * (double)k / (double)N;
    ::sincos(a, &tw[2 * (size_t)k + 1], &tw[2 * (size_t)k]);
  }
}

inline void nr_freqs(uint32_t fs, int n, std::vector<double> &f) {  // np.fft.rfftfreq(n, 1 / fs)
  const double d = 1.0 / (double)fs, val = 1.0 / ((double)n * d);
  f.resize((size_t)(n / 2 + 1));
  for (int k = 0; k <= n / 2; ++k) f[(size_t)k] = (double)k * val;
}

inline void nr_make_bands(uint32_t fs, const std::vector<double> &freqs, NrBandTable &t) {  // :138-145
  static const double centres[kNrBands] = {125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0, 8000.0};
  t = NrBandTable{};
  for (int b = 0; b < kNrBands; ++b) {
    const double low = centres[b] / std::sqrt(2.0), up = centres[b] * std::sqrt(2.0), cap = (double)fs * 0.49;
    const double high = up < cap ? up : cap;
    int first = -1, last = -1;
    for (int k = 0; k < (int)freqs.size(); ++k)
      if (freqs[(size_t)k] >= low && freqs[(size_t)k] < high) { if (first < 0) first = k; last = k; }
    if (first < 0) continue;
    t.first[t.n_bands] = first;
    t.last[t.n_bands] = last;
    ++t.n_bands;
  }
}

// per stream over audio[s][0 .. n): NrSampleStats; one wave a stream, lane l takes samples l, l + 64, ..., then an xor tree
hipError_t launch_nr_sample_stats(const float *audio, int64_t stride, int64_t n, int32_t n_streams, NrSampleStats *stats,
                                  hipStream_t stream);
// sums of x and x^2 (f64, non-finite samples as 0) over every hop-sized chunk: sums[(stream * n_chunks + chunk) * 2 + {0, 1}]
hipError_t launch_nr_chunk_sums(const float *audio, int64_t stride, int32_t n_streams, int32_t n_chunks, int32_t hop, double *sums,
                                hipStream_t stream);
// power[stream * n_frames + f] = mean((x - mean)^2) over frame f (chunks f, f + 1), mean = (sums[f] + sums[f + 1]) / N, :127-128
hipError_t launch_nr_frame_power(const float *audio, int64_t stride, const double *sums, int32_t n_streams, int32_t n_frames,
                                 int32_t hop, double *power, hipStream_t stream);
// per item: |rfft((x - mean) w)|^2 / sumw2 into psd[item.row][M + 1] and its sums over the octave bands into
// band_power[item.row][kNrBands] (the first bands.n_bands entries, 0 behind them).  twiddles: nr_make_twiddles(2 M).
hipError_t launch_nr_frame_spectra(const float *noise, int64_t noise_stride, const double *noise_sums, int32_t noise_chunks,
                                   const float *voice, int64_t voice_stride, const double *voice_sums, int32_t voice_chunks,
                                   const NrFrameItem *items, int32_t n_items, int32_t frame, const NrPlan &plan, const NrBandTable &bands,
                                   const double *window, const double *twiddles, double sumw2, double *psd, double *band_power,
                                   hipStream_t stream);

}  // namespace af
