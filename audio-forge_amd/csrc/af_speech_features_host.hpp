// af_speech_features_host.hpp -- what the host side and the kernels of the speech-feature measurement (af_speech_features.hip)
// share: the frame geometry of python/mic_eq/analysis/voice_setup.py:161-458 at 48 kHz, the BS.1770 coefficients of :133-136,
// the band table the host computes in f64, the work records and the launchers.  The Hann window, twiddles and factor list are
// af_noise_reference_host.hpp's (nr_make_window, nr_make_twiddles, nr_make_plan) for a frame of 1920.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "af_noise_reference_host.hpp"

namespace af {

constexpr int kSfFrame = 1920, kSfHop = 960;  // FRAME_MS 40, HOP_MS 20 at 48 kHz
constexpr int kSfMaxHop = 1920;               // 96 kHz: the largest half-frame the frame kernel takes (30 KB of LDS)
constexpr int kSfThreads = 256;
constexpr int kSfResampleThreads = 320;       // sf_resample_kernel: three outputs a thread over a chunk of 960
constexpr int kSfResampleSpan = 2048;         // inputs a chunk of 960 outputs reaches, at the most: 1963 at 96 kHz (2 x 16 KB of LDS)
constexpr int kSfBands = 6;        // low, body, presence, sibilance (:271-276), 250-4500 and 5000-9500 Hz (:305-308)
constexpr int kSfBandFields = 8;   // the six sums | the maximum of the last band | 0
constexpr int kSfSibBand = 5;      // the band whose bins go to the scratch row
constexpr int kSfTileStreams = 64;
// :133-136, the literal BS.1770 sections: b0 b1 b2 a1 a2 of the shelf, then of the high-pass
constexpr double kSfShelf[5] = {1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585};
constexpr double kSfHighpass[5] = {1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621};

// bins first[b] .. last[b] of each band (low <= f <= high, :284); the 5000-9500 Hz band holds sib_bins of them
struct SfBandTable { int32_t first[kSfBands], last[kSfBands]; };
// one frame: the one of `source` (1 the speech capture, 0 the noise capture) that starts at chunk `chunk`, into row `row` of
// the speech scratch (band sums, middles, arg-max, sibilance row) or of the noise sums
struct SfFrameItem { int32_t source, stream, chunk, row; };
// one candidate spectrum: rows [row0, row0 + count) of the sibilance scratch with their weights -> row `out`
struct SfPeakJob { int32_t row0, count, out, pad; };

// resample_poly's figures (sfm_geometry): output o reads input (o + rem) down / up and the ones before it, taps of phase
// (o + rem) down % up
struct SfResamplePlan { int32_t up, down, rem, taps; };
inline int sf_resample_span(const SfResamplePlan &p) { return (int)(((int64_t)(kSfHop - 1) * p.down + p.up - 1) / p.up) + p.taps; }

inline void sf_make_bands(uint32_t fs, const std::vector<double> &freqs, SfBandTable &t) {
  static const double low[kSfBands] = {80.0, 250.0, 2000.0, 5000.0, 250.0, 5000.0};
  double high[kSfBands] = {250.0, 2000.0, 5000.0, 10000.0, 4500.0, 9500.0};
  const double cap = (double)fs * 0.45;  // min(., 0.45 fs), :275 and :306-308: binds at 16 kHz only
  if (cap < high[3]) high[3] = cap;
  if (cap < high[5]) high[5] = cap;
  for (int b = 0; b < kSfBands; ++b) {
    t.first[b] = 0; t.last[b] = -1;
    for (int k = 0, seen = 0; k < (int)freqs.size(); ++k)
      if (freqs[(size_t)k] >= low[b] && freqs[(size_t)k] <= high[b]) { if (!seen) { t.first[b] = k; seen = 1; } t.last[b] = k; }
  }
}

// power[stream * n_frames + f] = mean(x^2) over frame f, not centred (:178); one wave a frame, lanes strided, xor tree
hipError_t launch_sf_frame_power(const float *audio, int64_t stride, int32_t n_streams, int32_t n_frames, int32_t frame, int32_t hop,
                                 double *power, hipStream_t stream);
// energy[stream * n_chunks + c] = sum(y^2) over hop-sized chunk c (the last may be partial) of the K-weighted capture: two
// cascaded sections in lfilter's transposed direct form II, shelf first; a lane per stream over 64-sample LDS tiles, 64 streams a
// workgroup, or down to 16 while that leaves fewer workgroups than compute units
hipError_t launch_sf_kweight(const float *audio, int64_t stride, int64_t n, int32_t n_streams, int32_t n_chunks, double *energy,
                             hipStream_t stream);
// the same over one segment of the resampled captures, signal[stream][row] (f64) holding the n samples from chunk chunk0 on (a
// whole number of chunks, but for the capture's end): energy[stream * n_chunks + c] for the segment's chunks, plus
// masked_energy likewise: the sum over the samples whose mask byte is set.  state[stream][4]: the two sections' states, taken
// up and left behind (zeros before the first segment)
hipError_t launch_sf_kweight_resampled(const double *signal, const uint8_t *mask, int64_t row, int64_t n, int32_t n_streams, int32_t n_chunks,
                                       int32_t chunk0, double *state, double *energy, double *masked_energy, hipStream_t stream);
// resample_poly(x, up, down) of audio[stream][0 .. n) and of the sample mask behind active[stream][n_frames]: the outputs of
// chunks chunk0 .. chunk0 + chunks (960 each, of the n48 there are) into signal[stream][row], mask[stream][row] (resampled mask
// >= 0.5) from column 0 on, and count[stream * ceil(n48 / 960) + c]; table: [up][taps]
hipError_t launch_sf_resample(const float *audio, int64_t stride, int64_t n, int32_t n_streams, const uint8_t *active, int32_t n_frames,
                              int32_t hop, const SfResamplePlan &plan, const double *table, int64_t n48, int32_t chunk0, int32_t chunks,
                              int64_t row, double *signal, uint8_t *mask, int32_t *count, hipStream_t stream);
// per item |rfft((x - mean) hanning)|^2 + 1e-18 over a frame of 2 hop samples (window [2 hop], twiddles nr_make_twiddles(2 hop)); a speech frame leaves band[row][kSfBandFields], the two middles of its
// 5000-9500 Hz bins in sib_mid[row][2], their first arg-max in sib_arg[row] and the bins in sib_rows[row][sib_bins]; a noise
// frame leaves the 5000-9500 Hz sum in noise_band[row]
hipError_t launch_sf_frames(const float *speech, int64_t speech_stride, const float *noise, int64_t noise_stride, const SfFrameItem *items,
                            int32_t n_items, int32_t hop, const NrPlan &plan, const SfBandTable &bands, const double *window, const double *twiddles,
                            double *band, double *sib_mid, int32_t *sib_arg, double *sib_rows, double *noise_band, hipStream_t stream);
// per job and bin: sum over the job's rows in order of weights[row] * sib_rows[row][bin] into sums[out][sib_bins], and the
// first arg-max of that row into arg[out]
hipError_t launch_sf_weighted_peak(const double *sib_rows, const double *weights, const SfPeakJob *jobs, int32_t n_jobs, int32_t sib_bins,
                                   double *sums, int32_t *arg, hipStream_t stream);

}  // namespace af
