// af_spectrum_host.hpp -- what the host side and the kernels of the voice spectrum measurement (af_spectrum.hip) share: the
// constants of python/mic_eq/analysis/spectrum.py:17-25, the tables the host computes in f64 and uploads (window, twiddles,
// fractional-octave bands), the work records and the launchers.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>

#include <cmath>
#include <cstdint>
#include <vector>

namespace af {

constexpr double kVsRmsGateDb = -48.0;      // VOICE_FRAME_RMS_GATE_DB, spectrum.py:17
constexpr double kVsFloorPercentile = 20.0;  // :18
constexpr double kVsPeakPercentile = 95.0;   // :19
constexpr double kVsGateFraction = 0.60;     // :20
constexpr double kVsMinSpreadDb = 6.0;       // :21
constexpr double kVsMinVoicedRatio = 0.15;   // :22
constexpr int kVsMinVoicedFrames = 3;        // :23
constexpr int kVsSileroWindow = 512;         // :24
constexpr int kVsSileroRate = 16000;         // :25
constexpr double kVsVadEvidence = 0.4;       // VAD_SPEECH_EVIDENCE_THRESHOLD, analysis/vad.py
constexpr double kVsVadStrong = 0.65;        // VAD_STRONG_SPEECH_THRESHOLD
constexpr int kVsMinNperseg = 256, kVsMaxNperseg = 8192;
constexpr int kVsTileStreams = 64;           // window-spectra scratch is sized for at most this many streams
constexpr int kVsSmoothPasses = 3;           // 1/3, 1/6, 1/12 octave: what "balanced" reads (spectrum.py:959-967)
constexpr int kVsMaxBands = 160;             // 1/12 octave over 20 Hz .. 20 kHz has 120

constexpr int kVsBlockFrames = 3;           // UNCERTAINTY_BLOCK_FRAMES, :28
constexpr double kVsUncertaintyScaleDb = 2.5;  // UNCERTAINTY_SCALE_DB, :29
constexpr double kVsCoverageTargetBlocks = 12.0;  // PHONETIC_COVERAGE_TARGET_BLOCKS, :30
constexpr int kVsCoverageBands = 5;          // _coarse_phonetic_coverage's bands, :391-397
constexpr int kVsLevelFields = 2 + kVsCoverageBands;  // per smoothed window: voice-band mean | median | the band medians of S - mean

enum VsNoiseSource : int { kVsNoiseUnavailable = 0, kVsNoiseExplicit = 1, kVsNoiseInCapture = 2, kVsNoiseOverride = 3 };

// one window spectrum: the frame of `source` (0 the capture, 1 the noise capture) that starts at chunk `chunk`
struct VsWindowItem { int32_t source, stream, chunk, row; };
// one column median: rows [row0, row0 + count) of the scratch -> row `out` of the medians
struct VsMedianJob { int32_t row0, count, out, pad; };

// the bin ranges of the reliability statistics: the voice band 100 Hz <= f <= 8 kHz (every bin when it holds none, :265-267,
// :438-442) and the coverage bands low <= f < high (:391-400; last < first: the band holds no bin and is skipped)
struct VsBandTable { int32_t v0, v1, first[kVsCoverageBands], last[kVsCoverageBands]; };
// one column median with per-row offsets: over list[first .. first + count) (rows of the smoothed scratch) of
// S[row][k] - levels[row][which], plus `add` when `with_add`, into row `out`
struct VsOffsetJob { int32_t first, count, out, which; double add; int32_t with_add, pad; };
// the block rows [row0, row0 + count) of one stream -> row `out` of the uncertainty, the reliability and the block statistics
struct VsBlockJob { int32_t row0, count, out, pad; };

inline void vs_make_band_table(const std::vector<double> &freqs, VsBandTable &t) {
  static const double edges[kVsCoverageBands + 1] = {100.0, 350.0, 1000.0, 2500.0, 4500.0, 8000.0};
  const int K = (int)freqs.size();
  t.v0 = 0; t.v1 = -1;
  for (int k = 0, seen = 0; k < K; ++k)
    if (freqs[(size_t)k] >= 100.0 && freqs[(size_t)k] <= 8000.0) { if (!seen) { t.v0 = k; seen = 1; } t.v1 = k; }
  if (t.v1 < t.v0) { t.v0 = 0; t.v1 = K - 1; }
  for (int b = 0; b < kVsCoverageBands; ++b) {
    t.first[b] = 0; t.last[b] = -1;
    for (int k = 0, seen = 0; k < K; ++k)
      if (freqs[(size_t)k] >= edges[b] && freqs[(size_t)k] < edges[b + 1]) { if (!seen) { t.first[b] = k; seen = 1; } t.last[b] = k; }
  }
}

// a fractional-octave pass on the FFT grid: the bands that hold a bin (spectrum.py:917-932 `valid`)
struct VsSmoothTables {
  int32_t n_bands[kVsSmoothPasses] = {};
  std::vector<double> centre[kVsSmoothPasses];
  std::vector<int32_t> first[kVsSmoothPasses], last[kVsSmoothPasses];
  std::vector<int32_t> bin_pass, bin_index;  // per bin: the pass its region reads; the band below it, -1 left, -2 right, -3 copy
  std::vector<double> freqs;
};

inline void vs_make_window(int N, std::vector<double> &w, double *sumw2) {  // np.hamming(N), symmetric
  const double pi = 3.14159265358979323846;
  w.resize((size_t)N);
  double s = 0.0;
  for (int i = 0; i < N; ++i) {
    w[(size_t)i] = 0.54 + 0.46 * std::cos(pi * (double)(2 * i + 1 - N) / (double)(N - 1));
    s += w[(size_t)i] * w[(size_t)i];
  }
  *sumw2 = s;
}

// signal.welch's get_window("hamming", N): periodic, the symmetric window of N + 1 points without its last
inline void vs_make_welch_window(int N, std::vector<double> &w, double *sumw2) {
  const double pi = 3.14159265358979323846, step = (pi - (-pi)) / (double)N;  // np.linspace(-pi, pi, N + 1)
  w.resize((size_t)N);
  double s = 0.0;
  for (int i = 0; i < N; ++i) {
    w[(size_t)i] = 0.54 + 0.46 * std::cos((double)i * step + (-pi));
    s += w[(size_t)i] * w[(size_t)i];
  }
  *sumw2 = s;
}

inline void vs_make_twiddles(int N, std::vector<double> &tw) {  // exp(-2 pi i k / N), k = 0 .. N/2, (re, im) pairs
  const double pi = 3.14159265358979323846;
  tw.resize(2 * (size_t)(N / 2 + 1));
  for (int k = 0; k <= N / 2; ++k) {
    const double a = -2.0 * pi * (double)k / (double)N;
    ::sincos(a, &tw[2 * (size_t)k + 1], &tw[2 * (size_t)k]);  // one libm entry whatever the compiler would merge cos() and sin() into
  }
}

inline void vs_freqs(uint32_t fs, int N, std::vector<double> &f) {  // np.fft.rfftfreq(N, 1 / fs)
  const double d = 1.0 / (double)fs, val = 1.0 / ((double)N * d);
  f.resize((size_t)(N / 2 + 1));
  for (int k = 0; k <= N / 2; ++k) f[(size_t)k] = (double)k * val;
}

// get_octave_frequencies(fraction) with its default limits and reference, spectrum.py:839-889
inline int vs_octave_bands(int b, std::vector<double> &centre, std::vector<double> &lower, std::vector<double> &upper) {
  const double G = std::pow(10.0, 0.3);
  const int x_min = (int)std::floor((double)b * std::log10(20.0 / 1000.0) / std::log10(G));
  const int x_max = (int)std::ceil((double)b * std::log10(20000.0 / 1000.0) / std::log10(G));
  centre.clear(); lower.clear(); upper.clear();
  for (int x = x_min; x <= x_max; ++x) {
    const double fm = (b % 2 == 1) ? 1000.0 * std::pow(G, (double)x / (double)b)
                                   : 1000.0 * std::pow(G, (double)(2 * x + 1) / (double)(2 * b));
    if (20.0 <= fm && fm <= 20000.0) {
      const double h = std::pow(G, 1.0 / (double)(2 * b));
      centre.push_back(fm);
      lower.push_back(fm / h);
      upper.push_back(fm * h);
    }
  }
  return (int)centre.size();
}

inline void vs_make_smooth_tables(uint32_t fs, int N, VsSmoothTables &t) {
  static const int fractions[kVsSmoothPasses] = {3, 6, 12};
  const int K = N / 2 + 1;
  vs_freqs(fs, N, t.freqs);
  for (int p = 0; p < kVsSmoothPasses; ++p) {
    std::vector<double> c, lo, up;
    const int nb = vs_octave_bands(fractions[p], c, lo, up);
    t.centre[p].clear(); t.first[p].clear(); t.last[p].clear();
    for (int b = 0; b < nb; ++b) {
      int first = -1, last = -1;
      for (int k = 0; k < K; ++k)
        if (t.freqs[(size_t)k] >= lo[(size_t)b] && t.freqs[(size_t)k] <= up[(size_t)b]) { if (first < 0) first = k; last = k; }
      if (first < 0) continue;
      t.centre[p].push_back(c[(size_t)b]);
      t.first[p].push_back(first);
      t.last[p].push_back(last);
    }
    t.n_bands[p] = (int32_t)t.centre[p].size();
  }
  t.bin_pass.resize((size_t)K);
  t.bin_index.resize((size_t)K);
  for (int k = 0; k < K; ++k) {
    const double f = t.freqs[(size_t)k];
    const int p = f < 180.0 ? 0 : (f < 3500.0 ? 1 : (f <= 9000.0 ? 2 : 0));  // spectrum.py:959-967
    const std::vector<double> &xc = t.centre[p];
    const int n = t.n_bands[p];
    int idx;
    if (n <= 1) idx = -3;  // :943-944: the pass returns the spectrum itself
    else if (f < xc[0]) idx = -1;
    else if (f >= xc[(size_t)n - 1]) idx = -2;
    else {
      int lo = 0, hi = n - 1;
      while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        if (f >= xc[(size_t)mid]) lo = mid; else hi = mid;
      }
      idx = lo;
    }
    t.bin_pass[(size_t)k] = p;
    t.bin_index[(size_t)k] = idx;
  }
}

// sums of x and x^2 (f64) over every hop-sized chunk: sums[(stream * n_chunks + chunk) * 2 + {0, 1}]
hipError_t launch_vs_chunk_sums(const float *audio, int64_t stride, int32_t n_streams, int32_t n_chunks, int32_t hop, double *sums,
                                hipStream_t stream);
// window spectra: |rfft((x - mean) w)|^2 / sumw2 into linear[item.row][bins]; db (nullable) takes 10 log10(. + 1e-12) of it
hipError_t launch_vs_window_spectra(const float *audio, int64_t stride, const double *sums, int32_t n_chunks, const float *noise,
                                    int64_t noise_stride, const double *noise_sums, int32_t noise_chunks, const VsWindowItem *items,
                                    int32_t n_items, int32_t nperseg, const double *window, const double *twiddles, double sumw2,
                                    double *db, double *linear, hipStream_t stream);
// Welch: stream s sums |X|^2 over segments (chunks[offset[s] + j], chunks[offset[s] + j + 1]), j in order, into
// sum[s][bins], then 10 log10(sum * scale (* 2 inside) / segments + 1e-12) into db[s][bins]
hipError_t launch_vs_welch(const float *audio, int64_t stride, const double *sums, int32_t n_chunks, const int32_t *chunks,
                           const int32_t *offset, int32_t n_streams, int32_t nperseg, const double *window, const double *twiddles,
                           double scale, double *sum, double *db, hipStream_t stream);
// the middle value(s) of every column of row ranges of rows[.][bins] (the linear PSD: the dB is monotone, so the median only
// selects): out[job.out][0][bins] the lower middle, out[job.out][1][bins] the upper one (the same for an odd count).  The host
// takes their dB with its own log10 and NumPy's even-count mean, so the medians carry the host libm's bits.
hipError_t launch_vs_median(const double *rows, const VsMedianJob *jobs, int32_t n_jobs, int32_t bins, double *out, hipStream_t stream);
// perceptual smoothing of rows[row_index[i]][bins] into out[i][bins]; tables as VsSmoothTables, passes back to back
hipError_t launch_vs_smooth(const double *rows, const int32_t *row_index, int32_t n_rows, int32_t bins, const int32_t *n_bands,
                            const double *centre, const int32_t *first, const int32_t *last, const int32_t *bin_pass,
                            const int32_t *bin_index, const double *freqs, double *out, hipStream_t stream);

// ---- reliability statistics (af_spectrum_stats.hip): the second half of analyze_voice_spectrum, spectrum.py:250-290, 381-495
// levels[row][kVsLevelFields] of every smoothed row: mean and median over the voice band, and the coverage bands' medians of
// S - mean (NaN for a band without a bin)
hipError_t launch_vs_row_levels(const double *smooth, int32_t n_rows, int32_t bins, const VsBandTable &bands, double *levels,
                                hipStream_t stream);
// per (job, bin) the median (np.median: the mean of both middles for an even count) over the job's row list
hipError_t launch_vs_offset_median(const double *smooth, const int32_t *list, const double *levels, const VsOffsetJob *jobs,
                                   int32_t n_jobs, int32_t bins, double *out, hipStream_t stream);
// distance[row] = sqrt(mean over the voice band of (S - median level - centres[row_centre[row]])^2); NaN where row_centre < 0
hipError_t launch_vs_shape_distance(const double *smooth, int32_t n_rows, int32_t bins, const VsBandTable &bands, const double *levels,
                                    const int32_t *row_centre, const double *centres, double *distance, hipStream_t stream);
// per job: stats[out][4] = lag-one dot product, left and right squared norms of the blocks minus their column median, effective
// block count (:411-424); uncertainty[out][bins] (:470-477) and reliability[out][bins] (:478, clipped); +inf and 0 below two blocks
hipError_t launch_vs_block_stats(const double *block_rows, const VsBlockJob *jobs, int32_t n_jobs, int32_t bins, double *uncertainty,
                                 double *reliability, double *stats, hipStream_t stream);

}  // namespace af
