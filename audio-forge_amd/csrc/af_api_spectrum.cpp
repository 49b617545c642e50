// af_api_spectrum.cpp -- the C ABI of the batched voice spectrum measurement (af_voice_spectrum_*): python/mic_eq/analysis/
// spectrum.py:69-343, 519-645, 839-967.  The kernels do what is O(samples) and O(frames x bins); everything that is O(frames)
// per stream (percentiles, the two gates, the VAD fusion, the choice of noise reference, the fallback decision) is decided here
// between the energy pass and the spectra.  Kernels and tables: af_spectrum.hip / af_spectrum_host.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "af_api_internal.hpp"
#include "af_numpy_rules.h"
#include "af_spectrum_host.hpp"

struct af_voice_spectrum {
  int device = 0, nperseg = 0, bins = 0;
  uint32_t sample_rate = 0;
  bool touched_device = false;
  double sumw2 = 0.0, welch_sumw2 = 0.0;
  std::vector<double> window, welch_window, twiddles;  // np.hamming (symmetric) | signal.welch's periodic Hamming
  af::VsSmoothTables smooth;
  // uploaded at the first call
  af::DeviceBuffer<double> d_window, d_welch_window, d_twiddles, d_centre, d_freqs;
  af::DeviceBuffer<int32_t> d_bands;  // n_bands[3] | first[3][kVsMaxBands] | last[3][kVsMaxBands] | bin_pass[bins] | bin_index[bins]
  // per call
  af::DeviceBuffer<float> d_audio, d_noise;  // staging of the host entry point
  af::DeviceBuffer<double> d_sums, d_noise_sums, d_welch_sum, d_welch_db;
  af::DeviceBuffer<int32_t> d_chunks, d_offset, d_smooth_rows;
  // per tile of streams
  af::DeviceBuffer<double> d_rows_db, d_rows_linear, d_rows_smooth, d_medians;
  af::DeviceBuffer<af::VsWindowItem> d_items;
  af::DeviceBuffer<af::VsMedianJob> d_jobs;
  af::EventChain events;  // pairs of marks around the kernels of the last call
  std::vector<int8_t> span_kind;  // per pair from the first reliability span on: which kernel of af_spectrum_stats.hip it times
  // the voiced frames' spectra of the last call that kept them
  bool have_windows = false;
  std::vector<int64_t> win_offset;  // [n_streams + 1] rows
  std::vector<double> win_raw, win_smooth, win_linear;
  // the reliability statistics (af_spectrum_stats.hip): opt-in; scratch per tile, results of the last call that computed them
  bool reliability = false, have_reliability = false;
  af::VsBandTable bands = {};
  af::DeviceBuffer<double> d_levels, d_distance, d_rel_medians, d_rel_robust, d_rel_uncertainty, d_rel_repeat, d_rel_stats;
  af::DeviceBuffer<int32_t> d_rel_list, d_row_centre;
  af::DeviceBuffer<af::VsOffsetJob> d_rel_jobs;
  af::DeviceBuffer<af::VsBlockJob> d_block_jobs;
  int32_t rel_streams = 0, rel_frames = 0;
  std::vector<af_voice_spectrum_reliability_row> rel_rows;
  std::vector<double> rel_median, rel_repeat, rel_uncertainty, rel_snr, rel_distance;
  std::vector<uint8_t> rel_inlier;
  // the noise-spectrum override (af_voice_spectrum_set_noise_override): a copy of the caller's arrays, none when ov_points is 0
  int32_t ov_points = 0, ov_streams = 0;
  bool ov_shared = false;
  std::vector<double> ov_freqs, ov_db;  // [ov_points] | [ov_shared ? 1 : ov_streams][ov_points]
  ~af_voice_spectrum() {
    if (touched_device) { (void)hipSetDevice(device); (void)hipDeviceSynchronize(); }
  }
};

namespace {

double vs_percentile_sorted(const std::vector<double> &s, double q) {  // np.percentile, method "linear"
  return af_percentile_sorted(s.data(), (int)s.size(), q);  // the one restatement of the rule, af_numpy_rules.h
}

double vs_median(std::vector<double> v) {  // np.median
  std::sort(v.begin(), v.end());
  const size_t n = v.size();
  return n % 2 ? v[n / 2] : (v[n / 2 - 1] + v[n / 2]) / 2.0;
}

double vs_interp(double x, const double *xp, const double *fp, int n) {  // np.interp, ends held
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

// the override of one stream when it passes spectrum.py:557-563 (at least two points, all finite), else null
const double *vs_valid_override(const af_voice_spectrum *h, int stream) {
  if (h->ov_points < 2) return nullptr;
  const double *db = h->ov_db.data() + (h->ov_shared ? 0 : (size_t)stream * h->ov_points);
  for (int i = 0; i < h->ov_points; ++i)
    if (!std::isfinite(h->ov_freqs[(size_t)i]) || !std::isfinite(db[i])) return nullptr;
  return db;
}

// what the host decides for one stream from its frame levels
struct VsDecision {
  std::vector<double> rms;
  std::vector<uint8_t> mask;
  std::vector<int32_t> chunks;  // the hop-sized chunks compute_voice_spectrum keeps
  int voiced = 0, source = af::kVsNoiseUnavailable;
  bool vad_used = false, fallback = false;
  double ratio = 0.0, vad_active = 0.0;
};

void vs_decide(const double *sums /* [C][2] */, int F, int N, uint32_t fs, const double *vad, int64_t n_vad, bool explicit_noise,
               bool override_noise, VsDecision &d) {
  const int hop = N / 2, C = F + 1;
  d.rms.resize((size_t)F);
  d.mask.assign((size_t)F, 0);
  for (int f = 0; f < F; ++f) {  // _frame_rms_db, spectrum.py:167-169
    const double power = (sums[2 * f + 1] + sums[2 * (f + 1) + 1]) / (double)N;
    d.rms[(size_t)f] = 10.0 * std::log10(power + 1e-12);
  }
  std::vector<double> sorted(d.rms);
  std::sort(sorted.begin(), sorted.end());
  const double floor_db = vs_percentile_sorted(sorted, af::kVsFloorPercentile);
  const double peak_db = vs_percentile_sorted(sorted, af::kVsPeakPercentile);
  const double spread = peak_db - floor_db, wide = std::max(spread, af::kVsMinSpreadDb);

  // _voiced_frame_mask, :200-247
  const double gate = std::max(af::kVsRmsGateDb, floor_db + af::kVsGateFraction * wide);
  for (int f = 0; f < F; ++f) d.mask[(size_t)f] = spread < af::kVsMinSpreadDb ? 1 : (d.rms[(size_t)f] >= gate);
  d.vad_used = false;
  d.vad_active = 0.0;
  if (vad && n_vad > 0) {  // _interpolate_vad_probabilities, :172-197
    std::vector<double> xp((size_t)n_vad), fp((size_t)n_vad), posts((size_t)F);
    const int64_t win = std::max<int64_t>(1, (int64_t)std::ceil((double)fs * (double)af::kVsSileroWindow / (double)af::kVsSileroRate));
    af_interpolate_vad_probabilities(vad, n_vad, win, F, hop, N, xp.data(), fp.data(), posts.data());  // shared with the speech features
    const double support = std::max(af::kVsRmsGateDb, floor_db + 0.25 * wide);
    std::vector<uint8_t> combined((size_t)F);
    int count = 0, active = 0;
    for (int f = 0; f < F; ++f) {
      const double post = posts[(size_t)f];
      active += post >= af::kVsVadEvidence;
      combined[(size_t)f] = (post >= af::kVsVadEvidence && d.rms[(size_t)f] >= support) || post >= af::kVsVadStrong;
      count += combined[(size_t)f];
    }
    if (count >= af::kVsMinVoicedFrames) d.mask = combined;
    d.vad_used = true;
    d.vad_active = (double)active / (double)F;
  }
  d.voiced = 0;
  for (int f = 0; f < F; ++f) d.voiced += d.mask[(size_t)f];
  d.ratio = (double)d.voiced / (double)F;

  // the noise reference, :570-586
  d.source = af::kVsNoiseUnavailable;
  if (override_noise) {  // :554-569: a valid override goes first
    d.source = af::kVsNoiseOverride;
  } else if (explicit_noise) {
    d.source = af::kVsNoiseExplicit;
  } else if (F - d.voiced >= af::kVsMinVoicedFrames && d.voiced > 0) {
    std::vector<double> lv, lu;
    for (int f = 0; f < F; ++f) (d.mask[(size_t)f] ? lv : lu).push_back(d.rms[(size_t)f]);
    if (vs_median(lv) - vs_median(lu) >= 3.0) d.source = af::kVsNoiseInCapture;
  }
  d.fallback = d.voiced < af::kVsMinVoicedFrames || d.ratio < af::kVsMinVoicedRatio;  // :605

  // _select_voiced_samples, :69-107: unions of frames that start on multiples of the hop, so whole chunks
  const double gate2 = std::max(af::kVsRmsGateDb, floor_db + af::kVsGateFraction * spread);
  bool whole = spread < af::kVsMinSpreadDb;
  if (!whole) {
    int count = 0;
    for (int f = 0; f < F; ++f) count += d.rms[(size_t)f] >= gate2;
    if (count < af::kVsMinVoicedFrames || (double)count / (double)F < af::kVsMinVoicedRatio) whole = true;
  }
  d.chunks.clear();
  for (int c = 0; c < C; ++c)
    if (whole || (c < F && d.rms[(size_t)c] >= gate2) || (c > 0 && d.rms[(size_t)c - 1] >= gate2)) d.chunks.push_back(c);
}

void vs_spectral_snr(const double *speech, const double *noise, int K, double *out) {  // _spectral_snr_db, :333-342
  for (int k = 0; k < K; ++k) {
    const double total = std::pow(10.0, speech[k] / 10.0);
    const double np = std::max(std::pow(10.0, noise[k] / 10.0), 1e-18);
    const double sig = std::max(total - np, np * 1e-6);
    out[k] = 10.0 * std::log10(sig / np);
  }
}

double vs_clip(double v, double lo, double hi) { return std::min(std::max(v, lo), hi); }

// _estimate_snr_from_spectrum, :345-365: the integrated SNR over 80 Hz .. 8 kHz (every bin when the band holds none)
double vs_estimate_snr(const std::vector<double> &freqs, const double *spectrum, const double *noise /* nullable */) {
  if (!noise) return 0.0;
  const int K = (int)freqs.size();
  bool any = false;
  for (int k = 0; k < K; ++k) any = any || (freqs[(size_t)k] >= 80.0 && freqs[(size_t)k] <= 8000.0);
  double noise_sum = 0.0, signal_sum = 0.0;
  for (int k = 0; k < K; ++k) {
    if (any && !(freqs[(size_t)k] >= 80.0 && freqs[(size_t)k] <= 8000.0)) continue;
    const double total = std::pow(10.0, spectrum[k] / 10.0), np = std::pow(10.0, noise[k] / 10.0);
    noise_sum += np;
    signal_sum += total - np;
  }
  noise_sum = std::max(noise_sum, 1e-18);
  signal_sum = std::max(signal_sum, noise_sum * 1e-6);
  return 10.0 * std::log10(signal_sum / noise_sum);
}

// _estimate_tilt_db_per_octave, :368-378: the least-squares slope over log2(f), 100 Hz .. 8 kHz
double vs_estimate_tilt(const std::vector<double> &freqs, const double *spectrum) {
  std::vector<double> x, y;
  for (size_t k = 0; k < freqs.size(); ++k)
    if (freqs[k] >= 100.0 && freqs[k] <= 8000.0) { x.push_back(std::log2(freqs[k])); y.push_back(spectrum[k]); }
  if (x.size() < 2) return 0.0;
  double mx = 0.0, my = 0.0, denom = 0.0, dot = 0.0;
  for (size_t i = 0; i < x.size(); ++i) { mx += x[i]; my += y[i]; }
  mx /= (double)x.size();
  my /= (double)y.size();
  for (size_t i = 0; i < x.size(); ++i) { x[i] -= mx; denom += x[i] * x[i]; }
  if (denom <= 0.0) return 0.0;
  for (size_t i = 0; i < x.size(); ++i) dot += x[i] * (y[i] - my);
  return dot / denom;
}

int vs_upload_tables(af_voice_spectrum *h) {
  if (h->d_window) return AF_OK;
  const size_t N = (size_t)h->nperseg, K = (size_t)h->bins, P = af::kVsSmoothPasses, MB = af::kVsMaxBands;
  std::vector<double> centre(P * MB, 0.0);
  std::vector<int32_t> tab(P + 2 * P * MB + 2 * K, 0);
  for (size_t p = 0; p < P; ++p) {
    tab[p] = h->smooth.n_bands[p];
    for (size_t b = 0; b < (size_t)h->smooth.n_bands[p]; ++b) {
      centre[p * MB + b] = h->smooth.centre[p][b];
      tab[P + p * MB + b] = h->smooth.first[p][b];
      tab[P + P * MB + p * MB + b] = h->smooth.last[p][b];
    }
  }
  std::copy(h->smooth.bin_pass.begin(), h->smooth.bin_pass.end(), tab.begin() + (long)(P + 2 * P * MB));
  std::copy(h->smooth.bin_index.begin(), h->smooth.bin_index.end(), tab.begin() + (long)(P + 2 * P * MB + K));
  AF_HIP(h->d_twiddles.reserve_exact(sizeof(double) * h->twiddles.size()));
  AF_HIP(hipMemcpy(h->d_twiddles, h->twiddles.data(), sizeof(double) * h->twiddles.size(), hipMemcpyHostToDevice));
  AF_HIP(h->d_welch_window.reserve_exact(sizeof(double) * N));
  AF_HIP(hipMemcpy(h->d_welch_window, h->welch_window.data(), sizeof(double) * N, hipMemcpyHostToDevice));
  AF_HIP(h->d_centre.reserve_exact(sizeof(double) * centre.size()));
  AF_HIP(hipMemcpy(h->d_centre, centre.data(), sizeof(double) * centre.size(), hipMemcpyHostToDevice));
  AF_HIP(h->d_freqs.reserve_exact(sizeof(double) * K));
  AF_HIP(hipMemcpy(h->d_freqs, h->smooth.freqs.data(), sizeof(double) * K, hipMemcpyHostToDevice));
  AF_HIP(h->d_bands.reserve_exact(sizeof(int32_t) * tab.size()));
  AF_HIP(hipMemcpy(h->d_bands, tab.data(), sizeof(int32_t) * tab.size(), hipMemcpyHostToDevice));
  AF_HIP(h->d_window.reserve_exact(sizeof(double) * N));  // last: its presence means "all tables are up"
  AF_HIP(h->d_window.keep_if(hipMemcpy(h->d_window, h->window.data(), sizeof(double) * N, hipMemcpyHostToDevice)));
  return AF_OK;
}

// every argument check of the two entry points; no HIP call
int vs_check(af_voice_spectrum *h, const float *audio, int64_t n_samples, int32_t n_streams, int64_t stride, const double *vad,
             int64_t n_vad, const float *noise, int64_t n_noise, int64_t noise_stride, const af_voice_spectrum_outputs *out) {
  if (!h) return fail(AF_ERR_INVALID_ARGUMENT, "voice spectrum handle is null");
  if (!audio) return fail(AF_ERR_INVALID_ARGUMENT, "audio is null");
  if (!out) return fail(AF_ERR_INVALID_ARGUMENT, "outputs is null");
  if (n_streams <= 0) return fail(AF_ERR_INVALID_ARGUMENT, "n_streams must be positive");
  if (n_samples < h->nperseg)  // spectrum.py:133-137, 519-523
    return fail(AF_ERR_INVALID_ARGUMENT, "Audio too short for FFT: need %d samples, got %lld (%.2f seconds)", h->nperseg,
                (long long)n_samples, (double)n_samples / (double)h->sample_rate);
  if (stride < n_samples) return fail(AF_ERR_INVALID_ARGUMENT, "stride must cover n_samples");
  if ((n_samples - h->nperseg) / (h->nperseg / 2) + 2 > (1 << 22)) return fail(AF_ERR_UNSUPPORTED, "more than 2^22 frames per stream");
  if (vad && n_vad <= 0) return fail(AF_ERR_INVALID_ARGUMENT, "vad_probabilities without a positive n_vad");
  if (!vad && n_vad > 0) return fail(AF_ERR_INVALID_ARGUMENT, "n_vad without vad_probabilities");
  if (noise && (n_noise < 0 || noise_stride < n_noise)) return fail(AF_ERR_INVALID_ARGUMENT, "noise_stride must cover n_noise >= 0");
  if (!noise && n_noise > 0) return fail(AF_ERR_INVALID_ARGUMENT, "n_noise without noise_audio");
  if (h->ov_points > 0 && !h->ov_shared && h->ov_streams != n_streams)
    return fail(AF_ERR_INVALID_ARGUMENT, "the noise override was set for %d streams, the call has %d", h->ov_streams, n_streams);
  return AF_OK;
}

// The reliability statistics of the streams [t0, t1) of one tile, spectrum.py:647-742, from the V smoothed rows in
// h->d_rows_smooth (stream s starts at row smooth_first[s - t0]).  Group A: row levels, the block and centre medians, the shape
// distances and the block statistics, with no round trip between them.  The host then decides the inliers (:276-289) and group B
// takes the robust median over them; everything O(windows) and the scalars of :673-721 are computed here.
// medians: the tile's [stream][speech | noise][bins] references.
int vs_reliability_tile(af_voice_spectrum *h, const std::vector<VsDecision> &dec, int t0, int t1, int F, const std::vector<int32_t> &smooth_first,
                        size_t V, const std::vector<double> &medians, hipStream_t q) {
  const int N = h->nperseg, hop = N / 2, K = h->bins, T = t1 - t0, LF = af::kVsLevelFields;
  const size_t row_bytes = sizeof(double) * (size_t)K;
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  static const double targets[af::kVsCoverageBands] = {3.0, 4.0, 5.0, 6.0, 7.0};  // :391-397
  struct Plan { int32_t sm0 = -1, blocks = 0, list_all = 0; std::vector<int32_t> independent; };
  std::vector<Plan> plans((size_t)T);
  std::vector<int32_t> list, row_centre(V, -1);
  std::vector<af::VsOffsetJob> jobs;
  std::vector<af::VsBlockJob> block_jobs;
  int32_t median_rows = 0;
  for (int s = t0; s < t1; ++s) {
    const VsDecision &d = dec[(size_t)s];
    Plan &p = plans[(size_t)(s - t0)];
    if (d.fallback) continue;
    p.sm0 = smooth_first[(size_t)(s - t0)];
    int64_t next_start = -1;
    for (int f = 0, j = 0; f < F; ++f) {  // :446-454: the voiced windows that do not overlap the one kept before
      if (!d.mask[(size_t)f]) continue;
      if ((int64_t)f * hop >= next_start) { p.independent.push_back(j); next_start = (int64_t)f * hop + N; }
      ++j;
    }
    const int32_t row0 = median_rows, whole = (int32_t)p.independent.size() / af::kVsBlockFrames;
    for (int32_t b = 0; b < whole; ++b) {  // :456-460: mean-level offsets
      jobs.push_back({(int32_t)list.size(), af::kVsBlockFrames, median_rows++, 0, 0.0, 0, 0});
      for (int i = 0; i < af::kVsBlockFrames; ++i) list.push_back(p.sm0 + p.independent[(size_t)(b * af::kVsBlockFrames + i)]);
    }
    if (whole == 0 && !p.independent.empty()) {  // :461-462
      jobs.push_back({(int32_t)list.size(), (int32_t)p.independent.size(), median_rows++, 0, 0.0, 0, 0});
      for (int32_t j : p.independent) list.push_back(p.sm0 + j);
    }
    p.blocks = median_rows - row0;
    block_jobs.push_back({row0, p.blocks, s - t0, 0});
    p.list_all = (int32_t)list.size();  // :270: the centre over all voiced windows, median-level offsets
    jobs.push_back({p.list_all, d.voiced, median_rows, 1, 0.0, 0, 0});
    for (int j = 0; j < d.voiced; ++j) { list.push_back(p.sm0 + j); row_centre[(size_t)(p.sm0 + j)] = median_rows; }
    ++median_rows;
  }
  std::vector<double> levels(V * (size_t)LF), distance(V), stats((size_t)T * 4);
  std::vector<double> robust((size_t)T * K), uncertainty((size_t)T * K), repeat((size_t)T * K);
  std::vector<uint8_t> inlier_of_row(V, 0);
  std::vector<uint8_t> closest((size_t)T, 0);
  std::vector<int32_t> n_inliers((size_t)T, 0);
  if (!jobs.empty()) {
    AF_HIP(h->d_levels.reserve_exact(sizeof(double) * levels.size()));
    AF_HIP(h->d_distance.reserve_exact(sizeof(double) * V));
    AF_HIP(h->d_row_centre.reserve_exact(sizeof(int32_t) * V));
    AF_HIP(h->d_rel_list.reserve_exact(sizeof(int32_t) * list.size()));
    AF_HIP(h->d_rel_jobs.reserve_exact(sizeof(af::VsOffsetJob) * jobs.size()));
    AF_HIP(h->d_block_jobs.reserve_exact(sizeof(af::VsBlockJob) * block_jobs.size()));
    AF_HIP(h->d_rel_medians.reserve_exact(row_bytes * (size_t)median_rows));
    AF_HIP(h->d_rel_robust.reserve_exact(row_bytes * (size_t)T));
    AF_HIP(h->d_rel_uncertainty.reserve_exact(row_bytes * (size_t)T));
    AF_HIP(h->d_rel_repeat.reserve_exact(row_bytes * (size_t)T));
    AF_HIP(h->d_rel_stats.reserve_exact(sizeof(double) * stats.size()));
    AF_HIP(hipMemcpy(h->d_row_centre, row_centre.data(), sizeof(int32_t) * V, hipMemcpyHostToDevice));
    AF_HIP(hipMemcpy(h->d_rel_list, list.data(), sizeof(int32_t) * list.size(), hipMemcpyHostToDevice));
    AF_HIP(hipMemcpy(h->d_rel_jobs, jobs.data(), sizeof(af::VsOffsetJob) * jobs.size(), hipMemcpyHostToDevice));
    AF_HIP(hipMemcpy(h->d_block_jobs, block_jobs.data(), sizeof(af::VsBlockJob) * block_jobs.size(), hipMemcpyHostToDevice));
    // a pair of marks per kernel (back to back on one stream: nothing waits for them), so that each one's share can be read
    const auto span = [&](int8_t kind) {
      h->span_kind.resize(h->events.marks() / 2, (int8_t)-1);
      h->span_kind.push_back(kind);
      return h->events.mark(q);
    };
    AF_HIP(span(0));
    AF_HIP(af::launch_vs_row_levels(h->d_rows_smooth, (int32_t)V, K, h->bands, h->d_levels, q));
    AF_HIP(h->events.mark(q));
    AF_HIP(span(1));
    AF_HIP(af::launch_vs_offset_median(h->d_rows_smooth, h->d_rel_list, h->d_levels, h->d_rel_jobs, (int32_t)jobs.size(), K,
                                       h->d_rel_medians, q));
    AF_HIP(h->events.mark(q));
    AF_HIP(span(2));
    AF_HIP(af::launch_vs_shape_distance(h->d_rows_smooth, (int32_t)V, K, h->bands, h->d_levels, h->d_row_centre, h->d_rel_medians,
                                        h->d_distance, q));
    AF_HIP(h->events.mark(q));
    AF_HIP(span(3));
    AF_HIP(af::launch_vs_block_stats(h->d_rel_medians, h->d_block_jobs, (int32_t)block_jobs.size(), K, h->d_rel_uncertainty,
                                     h->d_rel_repeat, h->d_rel_stats, q));
    AF_HIP(h->events.mark(q));
    AF_HIP(hipMemcpy(levels.data(), h->d_levels, sizeof(double) * levels.size(), hipMemcpyDeviceToHost));
    AF_HIP(hipMemcpy(distance.data(), h->d_distance, sizeof(double) * V, hipMemcpyDeviceToHost));
    AF_HIP(hipMemcpy(stats.data(), h->d_rel_stats, sizeof(double) * stats.size(), hipMemcpyDeviceToHost));

    // :276-289: the inliers of every stream, then the robust shape over them plus the inliers' median level
    jobs.clear();
    list.clear();
    for (int s = t0; s < t1; ++s) {
      const Plan &p = plans[(size_t)(s - t0)];
      if (p.sm0 < 0) continue;
      const int n = dec[(size_t)s].voiced;
      const double *dist = &distance[(size_t)p.sm0];
      const double mid = vs_median(std::vector<double>(dist, dist + n));
      std::vector<double> dev((size_t)n);
      for (int j = 0; j < n; ++j) dev[(size_t)j] = std::fabs(dist[j] - mid);
      const double cutoff = mid + 4.0 * std::max(vs_median(dev), 0.25);
      uint8_t *in = &inlier_of_row[(size_t)p.sm0];
      int count = 0;
      for (int j = 0; j < n; ++j) count += in[j] = dist[j] <= cutoff;
      const int minimum = std::max(3, (int)std::ceil((double)n * 0.50));
      if (count < minimum) {  // :281-285: the closest windows instead
        std::vector<int32_t> order((size_t)n);
        for (int j = 0; j < n; ++j) order[(size_t)j] = j;
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return dist[a] < dist[b]; });
        std::fill(in, in + n, (uint8_t)0);
        for (int j = 0; j < minimum && j < n; ++j) in[order[(size_t)j]] = 1;
        count = std::min(minimum, n);
        closest[(size_t)(s - t0)] = 1;
      }
      n_inliers[(size_t)(s - t0)] = count;
      std::vector<double> kept;
      const int32_t first = (int32_t)list.size();
      for (int j = 0; j < n; ++j)
        if (in[j]) { kept.push_back(levels[(size_t)(p.sm0 + j) * LF + 1]); list.push_back(p.sm0 + j); }
      jobs.push_back({first, count, s - t0, 1, vs_median(kept), 1, 0});
    }
    AF_HIP(hipMemcpy(h->d_rel_list, list.data(), sizeof(int32_t) * list.size(), hipMemcpyHostToDevice));
    AF_HIP(hipMemcpy(h->d_rel_jobs, jobs.data(), sizeof(af::VsOffsetJob) * jobs.size(), hipMemcpyHostToDevice));
    AF_HIP(span(4));
    AF_HIP(af::launch_vs_offset_median(h->d_rows_smooth, h->d_rel_list, h->d_levels, h->d_rel_jobs, (int32_t)jobs.size(), K,
                                       h->d_rel_robust, q));
    AF_HIP(h->events.mark(q));
    AF_HIP(hipMemcpy(robust.data(), h->d_rel_robust, row_bytes * (size_t)T, hipMemcpyDeviceToHost));
    AF_HIP(hipMemcpy(uncertainty.data(), h->d_rel_uncertainty, row_bytes * (size_t)T, hipMemcpyDeviceToHost));
    AF_HIP(hipMemcpy(repeat.data(), h->d_rel_repeat, row_bytes * (size_t)T, hipMemcpyDeviceToHost));
  }

  std::vector<double> welch, sorted;
  for (int s = t0; s < t1 && welch.empty(); ++s)
    if (dec[(size_t)s].fallback) {  // the fallback streams' Welch rows: one copy of the tile's
      welch.resize((size_t)T * K);
      AF_HIP(hipMemcpy(welch.data(), h->d_welch_db + (size_t)t0 * K, row_bytes * (size_t)T, hipMemcpyDeviceToHost));
    }
  for (int s = t0; s < t1; ++s) {
    const VsDecision &d = dec[(size_t)s];
    const Plan &p = plans[(size_t)(s - t0)];
    af_voice_spectrum_reliability_row &r = h->rel_rows[(size_t)s];
    double *median = &h->rel_median[(size_t)s * K], *rep = &h->rel_repeat[(size_t)s * K], *unc = &h->rel_uncertainty[(size_t)s * K];
    double *snr = &h->rel_snr[(size_t)s * K], *dist = &h->rel_distance[(size_t)s * F];
    uint8_t *inl = &h->rel_inlier[(size_t)s * F];
    const bool have_noise = d.voiced > 0 && d.source != af::kVsNoiseUnavailable;
    const double *noise = have_noise ? &medians[(size_t)(s - t0) * 2 * K + K] : nullptr;
    std::fill(dist, dist + F, nan);
    std::fill(inl, inl + F, (uint8_t)0);
    r = af_voice_spectrum_reliability_row{};
    if (p.sm0 < 0) {  // the fallback return, :606-645
      std::memcpy(median, &welch[(size_t)(s - t0) * K], row_bytes);
      std::fill(rep, rep + K, 0.0);
      std::fill(unc, unc + K, inf);
      if (noise) vs_spectral_snr(&medians[(size_t)(s - t0) * 2 * K], noise, K, snr);
      else std::fill(snr, snr + K, nan);
      r.snr_db = vs_estimate_snr(h->smooth.freqs, median, noise);
      r.spectral_tilt_db_per_octave = vs_estimate_tilt(h->smooth.freqs, median);
      r.measurement_coverage = 0.45;
      continue;
    }
    const int i = s - t0;
    std::memcpy(median, &robust[(size_t)i * K], row_bytes);
    std::memcpy(rep, &repeat[(size_t)i * K], row_bytes);
    std::memcpy(unc, &uncertainty[(size_t)i * K], row_bytes);
    for (int f = 0, j = 0; f < F; ++f)
      if (d.mask[(size_t)f]) { dist[f] = distance[(size_t)(p.sm0 + j)]; inl[f] = inlier_of_row[(size_t)(p.sm0 + j)]; ++j; }
    if (noise) vs_spectral_snr(median, noise, K, snr);  // :672
    else std::fill(snr, snr + K, nan);
    const double effective = stats[(size_t)i * 4 + 3];
    double diversity = 0.0;  // _coarse_phonetic_coverage over the independent windows, :381-408
    int scores = 0;
    for (int b = 0; b < af::kVsCoverageBands; ++b) {
      if (h->bands.last[b] < h->bands.first[b]) continue;
      sorted.clear();
      for (int32_t j : p.independent) sorted.push_back(levels[(size_t)(p.sm0 + j) * LF + 2 + b]);
      std::sort(sorted.begin(), sorted.end());
      const double spread = vs_percentile_sorted(sorted, 90.0) - vs_percentile_sorted(sorted, 10.0);
      diversity += vs_clip(spread / targets[b], 0.0, 1.0);
      ++scores;
    }
    diversity = scores ? diversity / (double)scores : 0.0;
    const double duration = vs_clip(effective / af::kVsCoverageTargetBlocks, 0.0, 1.0);  // :481-487, :685-691
    const double phonetic = std::sqrt(diversity * duration);
    const double inlier_ratio = (double)n_inliers[(size_t)i] / (double)std::max(1, d.voiced);
    const double snr_db = vs_estimate_snr(h->smooth.freqs, median, noise);
    const double score = vs_median(std::vector<double>(rep + h->bands.v0, rep + h->bands.v1 + 1));  // :679-684
    const double coverage = vs_clip(0.45 * inlier_ratio + 0.35 * phonetic + 0.20 * duration, 0.0, 1.0);
    double confidence;
    if (!noise) confidence = vs_clip(0.5625 * score + 0.4375 * phonetic, 0.0, 0.70);
    else confidence = vs_clip(0.45 * score + 0.35 * phonetic + 0.20 * vs_clip((snr_db - 3.0) / 15.0, 0.0, 1.0), 0.0, 1.0);
    r.snr_db = snr_db;
    r.spectral_tilt_db_per_octave = vs_estimate_tilt(h->smooth.freqs, median);
    r.residual_confidence = vs_clip(confidence * (0.75 + 0.25 * coverage), 0.0, 1.0);
    r.measurement_coverage = coverage;
    r.outlier_rejection_ratio = 1.0 - inlier_ratio;
    r.phonetic_coverage = phonetic;
    r.effective_measurement_blocks = effective;
    r.voiced = d.voiced;
    r.independent = (int32_t)p.independent.size();
    r.blocks = p.blocks;
    r.inliers = n_inliers[(size_t)i];
    r.used_closest_windows = closest[(size_t)i];
  }
  return AF_OK;
}

int vs_analyze(af_voice_spectrum *h, const float *d_audio, int64_t n, int32_t B, int64_t stride, const double *vad, int64_t n_vad,
               const float *d_noise, int64_t n_noise, int64_t noise_stride, const af_voice_spectrum_outputs *out) {
  const int N = h->nperseg, hop = N / 2, K = h->bins;
  const int F = (int)((n - N) / hop) + 1, C = F + 1;
  const bool explicit_noise = d_noise && n_noise >= N;  // _audio_reference_spectrum_db returns None below one frame, :326-327
  const int Fn = explicit_noise ? (int)((n_noise - N) / hop) + 1 : 0, Cn = explicit_noise ? Fn + 1 : 0;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  hipStream_t q = nullptr;
  h->have_windows = false;
  h->have_reliability = false;
  h->events.restart();
  h->span_kind.clear();
  if (int rc = vs_upload_tables(h)) return rc;

  // 1. chunk sums -> frame energies and means
  std::vector<double> sums((size_t)B * C * 2), nsums((size_t)B * Cn * 2);
  AF_HIP(h->d_sums.reserve_exact(sizeof(double) * sums.size()));
  if (explicit_noise) AF_HIP(h->d_noise_sums.reserve_exact(sizeof(double) * nsums.size()));
  AF_HIP(h->events.mark(q));
  AF_HIP(af::launch_vs_chunk_sums(d_audio, stride, B, C, hop, h->d_sums, q));
  if (explicit_noise) AF_HIP(af::launch_vs_chunk_sums(d_noise, noise_stride, B, Cn, hop, h->d_noise_sums, q));
  AF_HIP(h->events.mark(q));
  AF_HIP(hipMemcpy(sums.data(), h->d_sums, sizeof(double) * sums.size(), hipMemcpyDeviceToHost));
  if (explicit_noise) AF_HIP(hipMemcpy(nsums.data(), h->d_noise_sums, sizeof(double) * nsums.size(), hipMemcpyDeviceToHost));
  for (size_t i = 1; i < sums.size(); i += 2)
    if (!std::isfinite(sums[i])) return fail(AF_ERR_NON_FINITE, "audio must contain only finite samples");
  for (size_t i = 1; i < nsums.size(); i += 2)
    if (!std::isfinite(nsums[i])) return fail(AF_ERR_NON_FINITE, "noise_audio must contain only finite samples");

  // 2. the host's decisions, one stream at a time
  std::vector<VsDecision> dec((size_t)B);
  std::vector<int32_t> chunks, offset((size_t)B + 1, 0);
  for (int s = 0; s < B; ++s) {
    vs_decide(&sums[(size_t)s * C * 2], F, N, h->sample_rate, vad ? vad + (int64_t)s * n_vad : nullptr, n_vad, explicit_noise,
              vs_valid_override(h, s) != nullptr, dec[(size_t)s]);
    chunks.insert(chunks.end(), dec[(size_t)s].chunks.begin(), dec[(size_t)s].chunks.end());
    offset[(size_t)s + 1] = (int32_t)chunks.size();
  }

  // 3. Welch over the kept chunks, all streams
  AF_HIP(h->d_chunks.reserve_exact(sizeof(int32_t) * chunks.size()));
  AF_HIP(h->d_offset.reserve_exact(sizeof(int32_t) * offset.size()));
  AF_HIP(h->d_welch_sum.reserve_exact(sizeof(double) * (size_t)B * K));
  AF_HIP(h->d_welch_db.reserve_exact(sizeof(double) * (size_t)B * K));
  AF_HIP(hipMemcpy(h->d_chunks, chunks.data(), sizeof(int32_t) * chunks.size(), hipMemcpyHostToDevice));
  AF_HIP(hipMemcpy(h->d_offset, offset.data(), sizeof(int32_t) * offset.size(), hipMemcpyHostToDevice));
  AF_HIP(h->events.mark(q));
  AF_HIP(af::launch_vs_welch(d_audio, stride, h->d_sums, C, h->d_chunks, h->d_offset, B, N, h->d_welch_window, h->d_twiddles,
                             1.0 / ((double)h->sample_rate * h->welch_sumw2), h->d_welch_sum, h->d_welch_db, q));
  AF_HIP(h->events.mark(q));

  // 4. window spectra, medians and smoothing, a tile of streams at a time
  const bool keep = out->keep_windows != 0, reliability = h->reliability;
  if (reliability) {
    h->rel_streams = B;
    h->rel_frames = F;
    h->rel_rows.resize((size_t)B);
    for (std::vector<double> *v : {&h->rel_median, &h->rel_repeat, &h->rel_uncertainty, &h->rel_snr}) v->resize((size_t)B * K);
    h->rel_distance.resize((size_t)B * F);
    h->rel_inlier.resize((size_t)B * F);
  }
  if (keep) {
    h->win_offset.assign((size_t)B + 1, 0);
    for (int s = 0; s < B; ++s) h->win_offset[(size_t)s + 1] = h->win_offset[(size_t)s] + dec[(size_t)s].voiced;
    const size_t total = (size_t)h->win_offset[(size_t)B] * K;
    h->win_raw.resize(total);
    h->win_smooth.resize(total);
    h->win_linear.resize(total);
  }
  const size_t row_bytes = sizeof(double) * (size_t)K;
  const int64_t budget_rows = std::max<int64_t>(1, ((int64_t)256 << 20) / (int64_t)row_bytes);
  const int tile = (int)std::min<int64_t>(af::kVsTileStreams, std::max<int64_t>(1, budget_rows / (F + Fn)));
  const size_t P = af::kVsSmoothPasses, MB = af::kVsMaxBands;
  const int32_t *tb = h->d_bands;
  std::vector<double> medians, middle((size_t)2 * K);
  std::vector<af::VsWindowItem> items;
  std::vector<af::VsMedianJob> jobs;
  std::vector<int32_t> voiced_rows, first_row, smooth_first;
  for (int t0 = 0; t0 < B; t0 += tile) {
    const int t1 = std::min(B, t0 + tile);
    items.clear(); jobs.clear(); voiced_rows.clear(); first_row.clear(); smooth_first.clear();
    for (int s = t0; s < t1; ++s) {  // per stream: voiced frames | unvoiced frames (in-capture noise) | noise capture frames
      const VsDecision &d = dec[(size_t)s];
      const int32_t row0 = (int32_t)items.size();
      first_row.push_back(row0);
      const bool smoothed = keep || (reliability && !d.fallback);  // the windows vs_smooth_kernel takes
      smooth_first.push_back(smoothed ? (int32_t)voiced_rows.size() : -1);
      for (int f = 0; f < F; ++f)
        if (d.mask[(size_t)f]) {
          if (smoothed) voiced_rows.push_back((int32_t)items.size());
          items.push_back({0, s, f, (int32_t)items.size()});
        }
      if (d.voiced > 0) jobs.push_back({row0, d.voiced, 2 * (s - t0), 0});
      if (d.voiced > 0 && d.source == af::kVsNoiseInCapture) {
        const int32_t r = (int32_t)items.size();
        for (int f = 0; f < F; ++f)
          if (!d.mask[(size_t)f]) items.push_back({0, s, f, (int32_t)items.size()});
        jobs.push_back({r, F - d.voiced, 2 * (s - t0) + 1, 0});
      } else if (d.voiced > 0 && d.source == af::kVsNoiseExplicit) {
        const int32_t r = (int32_t)items.size();
        for (int f = 0; f < Fn; ++f) items.push_back({1, s, f, (int32_t)items.size()});
        jobs.push_back({r, Fn, 2 * (s - t0) + 1, 0});
      }
    }
    const size_t R = items.size(), V = voiced_rows.size();
    medians.assign((size_t)(t1 - t0) * 2 * K, nan);
    if (R > 0) {
      AF_HIP(h->d_rows_linear.reserve_exact(row_bytes * R));
      if (keep || reliability) AF_HIP(h->d_rows_db.reserve_exact(row_bytes * R));
      AF_HIP(h->d_items.reserve_exact(sizeof(af::VsWindowItem) * R));
      AF_HIP(h->d_jobs.reserve_exact(sizeof(af::VsMedianJob) * jobs.size()));
      AF_HIP(h->d_medians.reserve_exact(row_bytes * 4 * (size_t)(t1 - t0)));
      AF_HIP(hipMemcpy(h->d_items, items.data(), sizeof(af::VsWindowItem) * R, hipMemcpyHostToDevice));
      AF_HIP(hipMemcpy(h->d_jobs, jobs.data(), sizeof(af::VsMedianJob) * jobs.size(), hipMemcpyHostToDevice));
      if (V > 0) {
        AF_HIP(h->d_smooth_rows.reserve_exact(sizeof(int32_t) * V));
        AF_HIP(h->d_rows_smooth.reserve_exact(row_bytes * V));
        AF_HIP(hipMemcpy(h->d_smooth_rows, voiced_rows.data(), sizeof(int32_t) * V, hipMemcpyHostToDevice));
      }
      AF_HIP(h->events.mark(q));
      AF_HIP(af::launch_vs_window_spectra(d_audio, stride, h->d_sums, C, d_noise, noise_stride, h->d_noise_sums, Cn, h->d_items,
                                          (int32_t)R, N, h->d_window, h->d_twiddles, h->sumw2, keep || reliability ? h->d_rows_db.get() : nullptr,
                                          h->d_rows_linear, q));
      AF_HIP(af::launch_vs_median(h->d_rows_linear, h->d_jobs, (int32_t)jobs.size(), K, h->d_medians, q));
      if (V > 0)
        AF_HIP(af::launch_vs_smooth(h->d_rows_db, h->d_smooth_rows, (int32_t)V, K, tb, h->d_centre, tb + P, tb + P + P * MB,
                                    tb + P + 2 * P * MB, tb + P + 2 * P * MB + K, h->d_freqs, h->d_rows_smooth, q));
      AF_HIP(h->events.mark(q));
      for (const af::VsMedianJob &j : jobs) {  // rows no job wrote stay NaN
        AF_HIP(hipMemcpy(middle.data(), h->d_medians + (size_t)j.out * 2 * K, row_bytes * 2, hipMemcpyDeviceToHost));
        double *m = &medians[(size_t)j.out * K];
        for (int k = 0; k < K; ++k) {  // _window_spectrum_db's dB of the middle values, then np.median's mean of the two
          const double lo = 10.0 * std::log10(middle[(size_t)k] + 1e-12);
          const double hi = middle[(size_t)K + k] == middle[(size_t)k] ? lo : 10.0 * std::log10(middle[(size_t)K + k] + 1e-12);
          m[k] = (lo + hi) / 2.0;
        }
      }
      if (V > 0 && keep) {
        AF_HIP(hipMemcpy(&h->win_smooth[(size_t)h->win_offset[(size_t)t0] * K], h->d_rows_smooth, row_bytes * V, hipMemcpyDeviceToHost));
        for (int s = t0; s < t1; ++s) {
          const size_t cnt = (size_t)dec[(size_t)s].voiced, at = (size_t)h->win_offset[(size_t)s] * K;
          const size_t from = (size_t)first_row[(size_t)(s - t0)] * K;
          if (cnt == 0) continue;
          AF_HIP(hipMemcpy(&h->win_raw[at], h->d_rows_db + from, row_bytes * cnt, hipMemcpyDeviceToHost));
          AF_HIP(hipMemcpy(&h->win_linear[at], h->d_rows_linear + from, row_bytes * cnt, hipMemcpyDeviceToHost));
        }
      }
    }
    for (int s = t0; s < t1; ++s) {  // :596-602: the override on this grid, ends held
      const double *ov = dec[(size_t)s].source == af::kVsNoiseOverride && dec[(size_t)s].voiced > 0 ? vs_valid_override(h, s) : nullptr;
      if (!ov) continue;
      double *noise = &medians[(size_t)(s - t0) * 2 * K + K];
      for (int k = 0; k < K; ++k) noise[k] = vs_interp(h->smooth.freqs[(size_t)k], h->ov_freqs.data(), ov, h->ov_points);
    }
    for (int s = t0; s < t1; ++s) {
      const VsDecision &d = dec[(size_t)s];
      const double *speech = &medians[(size_t)(s - t0) * 2 * K], *noise = speech + K;
      const bool have_noise = d.voiced > 0 && d.source != af::kVsNoiseUnavailable;  // :594: both references exist
      if (out->speech_db) std::memcpy(out->speech_db + (size_t)s * K, speech, row_bytes);
      if (out->noise_db) std::memcpy(out->noise_db + (size_t)s * K, noise, row_bytes);
      if (out->spectral_snr_db) {
        double *snr = out->spectral_snr_db + (size_t)s * K;
        if (have_noise) vs_spectral_snr(speech, noise, K, snr);
        else std::fill(snr, snr + K, nan);
      }
    }
    if (reliability)
      if (int rc = vs_reliability_tile(h, dec, t0, t1, F, smooth_first, R > 0 ? V : 0, medians, q)) return rc;
  }
  if (out->welch_db) AF_HIP(hipMemcpy(out->welch_db, h->d_welch_db, row_bytes * (size_t)B, hipMemcpyDeviceToHost));
  if (out->welch_sum) AF_HIP(hipMemcpy(out->welch_sum, h->d_welch_sum, row_bytes * (size_t)B, hipMemcpyDeviceToHost));
  AF_HIP(hipStreamSynchronize(q));
  for (int s = 0; s < B; ++s) {
    const VsDecision &d = dec[(size_t)s];
    if (out->rows) {
      af_voice_spectrum_row &r = out->rows[s];
      r.frames = F;
      r.voiced = d.voiced;
      r.voiced_window_ratio = d.fallback ? std::max(d.ratio, 1.0 / (double)F) : d.ratio;  // :625, :726
      r.vad_active_window_ratio = d.vad_active;
      r.vad_probability_used = d.vad_used;
      r.noise_reference_source = d.source;
      r.used_single_spectrum_fallback = d.fallback;
      r.welch_segments = (int32_t)d.chunks.size() - 1;
    }
    for (int f = 0; f < F; ++f) {
      if (out->frame_power) out->frame_power[(size_t)s * F + f] = (sums[((size_t)s * C + f) * 2 + 1] + sums[((size_t)s * C + f + 1) * 2 + 1]) / (double)N;
      if (out->frame_rms_db) out->frame_rms_db[(size_t)s * F + f] = d.rms[(size_t)f];
      if (out->voiced_mask) out->voiced_mask[(size_t)s * F + f] = d.mask[(size_t)f];
    }
  }
  h->have_windows = keep;
  h->have_reliability = reliability;
  return AF_OK;
}

}  // namespace

extern "C" {

int af_voice_spectrum_create(uint32_t sample_rate, int32_t nperseg, int32_t device, af_voice_spectrum **out) {
  if (!out) return fail(AF_ERR_INVALID_ARGUMENT, "out is null");
  *out = nullptr;
  if (sample_rate == 0) return fail(AF_ERR_INVALID_ARGUMENT, "sample_rate must be positive");
  if (device < 0) return fail(AF_ERR_INVALID_ARGUMENT, "device must be >= 0");
  if (nperseg < af::kVsMinNperseg || nperseg > af::kVsMaxNperseg || (nperseg & (nperseg - 1)) != 0)
    return fail(AF_ERR_UNSUPPORTED, "nperseg %d: the transform is built for powers of two from %d to %d", nperseg, af::kVsMinNperseg,
                af::kVsMaxNperseg);
  af_voice_spectrum *h = new af_voice_spectrum();
  h->device = device;
  h->sample_rate = sample_rate;
  h->nperseg = nperseg;
  h->bins = nperseg / 2 + 1;
  af::vs_make_window(nperseg, h->window, &h->sumw2);
  af::vs_make_welch_window(nperseg, h->welch_window, &h->welch_sumw2);
  af::vs_make_twiddles(nperseg, h->twiddles);
  af::vs_make_smooth_tables(sample_rate, nperseg, h->smooth);
  af::vs_make_band_table(h->smooth.freqs, h->bands);
  *out = h;
  return AF_OK;
}

void af_voice_spectrum_destroy(af_voice_spectrum *h) { delete h; }

int32_t af_voice_spectrum_bins(const af_voice_spectrum *h) { return h ? h->bins : 0; }

int64_t af_voice_spectrum_frames(const af_voice_spectrum *h, int64_t n_samples) {
  if (!h || n_samples < h->nperseg) return 0;
  return (n_samples - h->nperseg) / (h->nperseg / 2) + 1;
}

int af_voice_spectrum_octave_bands(int32_t fraction, double *centre, double *lower, double *upper, int32_t capacity, int32_t *n_bands) {
  if (!n_bands) return fail(AF_ERR_INVALID_ARGUMENT, "n_bands is null");
  if (fraction < 1 || fraction > 48) return fail(AF_ERR_INVALID_ARGUMENT, "fraction must be 1 .. 48");
  std::vector<double> c, lo, up;
  *n_bands = af::vs_octave_bands(fraction, c, lo, up);
  if (*n_bands > capacity && (centre || lower || upper)) return fail(AF_ERR_INVALID_ARGUMENT, "%d bands do not fit %d", *n_bands, capacity);
  for (size_t b = 0; b < c.size(); ++b) {
    if (centre) centre[b] = c[b];
    if (lower) lower[b] = lo[b];
    if (upper) upper[b] = up[b];
  }
  return AF_OK;
}

int af_voice_spectrum_analyze_device(af_voice_spectrum *h, const float *d_audio, int64_t n_samples, int32_t n_streams, int64_t stride,
                                     const double *vad_probabilities, int64_t n_vad, const float *d_noise_audio, int64_t n_noise,
                                     int64_t noise_stride, const af_voice_spectrum_outputs *out) {
  if (int rc = vs_check(h, d_audio, n_samples, n_streams, stride, vad_probabilities, n_vad, d_noise_audio, n_noise, noise_stride, out))
    return rc;
  AF_HIP(hipSetDevice(h->device));
  h->touched_device = true;
  return vs_analyze(h, d_audio, n_samples, n_streams, stride, vad_probabilities, n_vad, d_noise_audio, n_noise, noise_stride, out);
}

int af_voice_spectrum_analyze_host(af_voice_spectrum *h, const float *audio, int64_t n_samples, int32_t n_streams, int64_t stride,
                                   const double *vad_probabilities, int64_t n_vad, const float *noise_audio, int64_t n_noise,
                                   int64_t noise_stride, const af_voice_spectrum_outputs *out) {
  if (int rc = vs_check(h, audio, n_samples, n_streams, stride, vad_probabilities, n_vad, noise_audio, n_noise, noise_stride, out))
    return rc;
  if (!af::check_finite(audio, n_streams, n_samples, stride)) return fail(AF_ERR_NON_FINITE, "audio must contain only finite samples");
  if (noise_audio && !af::check_finite(noise_audio, n_streams, n_noise, noise_stride))
    return fail(AF_ERR_NON_FINITE, "noise_audio must contain only finite samples");
  AF_HIP(hipSetDevice(h->device));
  h->touched_device = true;
  const size_t f4 = sizeof(float);
  AF_HIP(h->d_audio.reserve_exact(f4 * (size_t)n_streams * n_samples));  // (every call synchronises before it returns)
  AF_HIP(hipMemcpy2D(h->d_audio, f4 * n_samples, audio, f4 * stride, f4 * n_samples, n_streams, hipMemcpyHostToDevice));
  const bool with_noise = noise_audio && n_noise > 0;
  if (with_noise) {
    AF_HIP(h->d_noise.reserve_exact(f4 * (size_t)n_streams * n_noise));
    AF_HIP(hipMemcpy2D(h->d_noise, f4 * n_noise, noise_audio, f4 * noise_stride, f4 * n_noise, n_streams, hipMemcpyHostToDevice));
  }
  return vs_analyze(h, h->d_audio, n_samples, n_streams, n_samples, vad_probabilities, n_vad, with_noise ? h->d_noise.get() : nullptr,
                    with_noise ? n_noise : 0, n_noise, out);
}

int af_voice_spectrum_read_windows(af_voice_spectrum *h, int32_t stream, double *raw_db, double *smoothed_db, double *linear_psd,
                                   int32_t max_frames, int32_t *n_frames) {
  if (!h) return fail(AF_ERR_INVALID_ARGUMENT, "voice spectrum handle is null");
  if (!h->have_windows) return fail(AF_ERR_STATE, "the last call did not keep its window spectra (outputs.keep_windows)");
  if (stream < 0 || (size_t)stream + 1 >= h->win_offset.size()) return fail(AF_ERR_INVALID_ARGUMENT, "stream out of range");
  const int64_t cnt = h->win_offset[(size_t)stream + 1] - h->win_offset[(size_t)stream];
  if (n_frames) *n_frames = (int32_t)cnt;
  if (!raw_db && !smoothed_db && !linear_psd) return AF_OK;
  if (max_frames < cnt) return fail(AF_ERR_INVALID_ARGUMENT, "%lld voiced frames do not fit max_frames %d", (long long)cnt, max_frames);
  const size_t at = (size_t)h->win_offset[(size_t)stream] * h->bins, bytes = sizeof(double) * (size_t)cnt * h->bins;
  if (raw_db) std::memcpy(raw_db, h->win_raw.data() + at, bytes);
  if (smoothed_db) std::memcpy(smoothed_db, h->win_smooth.data() + at, bytes);
  if (linear_psd) std::memcpy(linear_psd, h->win_linear.data() + at, bytes);
  return AF_OK;
}

int af_voice_spectrum_set_reliability(af_voice_spectrum *h, int32_t enabled) {
  if (!h) return fail(AF_ERR_INVALID_ARGUMENT, "voice spectrum handle is null");
  h->reliability = enabled != 0;
  return AF_OK;
}

int af_voice_spectrum_set_noise_override(af_voice_spectrum *h, const double *freqs, const double *spectrum_db, int32_t n_points,
                                         int32_t n_streams, int64_t stride, int32_t shared) {
  if (!h) return fail(AF_ERR_INVALID_ARGUMENT, "voice spectrum handle is null");
  if (!spectrum_db) {  // clear
    h->ov_points = h->ov_streams = 0;
    h->ov_freqs.clear();
    h->ov_db.clear();
    return AF_OK;
  }
  if (!freqs) return fail(AF_ERR_INVALID_ARGUMENT, "freqs is null");
  if (n_points < 1) return fail(AF_ERR_INVALID_ARGUMENT, "n_points must be positive");
  if (!shared && (n_streams < 1 || stride < n_points)) return fail(AF_ERR_INVALID_ARGUMENT, "stride must cover n_points for n_streams >= 1");
  const int rows = shared ? 1 : n_streams;
  h->ov_freqs.assign(freqs, freqs + n_points);
  h->ov_db.resize((size_t)rows * n_points);
  for (int r = 0; r < rows; ++r) std::copy(spectrum_db + (int64_t)r * stride, spectrum_db + (int64_t)r * stride + n_points, &h->ov_db[(size_t)r * n_points]);
  h->ov_points = n_points;
  h->ov_streams = rows;
  h->ov_shared = shared != 0;
  return AF_OK;
}

int af_voice_spectrum_read_reliability(af_voice_spectrum *h, const af_voice_spectrum_reliability_outputs *out) {
  if (!h) return fail(AF_ERR_INVALID_ARGUMENT, "voice spectrum handle is null");
  if (!out) return fail(AF_ERR_INVALID_ARGUMENT, "outputs is null");
  if (!h->have_reliability)
    return fail(AF_ERR_STATE, "the last call did not compute the reliability statistics (af_voice_spectrum_set_reliability)");
  const size_t B = (size_t)h->rel_streams, K = (size_t)h->bins, F = (size_t)h->rel_frames;
  if (out->rows) std::copy(h->rel_rows.begin(), h->rel_rows.end(), out->rows);
  if (out->median_spectrum_db) std::memcpy(out->median_spectrum_db, h->rel_median.data(), sizeof(double) * B * K);
  if (out->spectral_repeatability) std::memcpy(out->spectral_repeatability, h->rel_repeat.data(), sizeof(double) * B * K);
  if (out->measurement_uncertainty_db) std::memcpy(out->measurement_uncertainty_db, h->rel_uncertainty.data(), sizeof(double) * B * K);
  if (out->spectral_snr_db) std::memcpy(out->spectral_snr_db, h->rel_snr.data(), sizeof(double) * B * K);
  if (out->window_distance) std::memcpy(out->window_distance, h->rel_distance.data(), sizeof(double) * B * F);
  if (out->inlier_mask) std::memcpy(out->inlier_mask, h->rel_inlier.data(), B * F);
  return AF_OK;
}

int af_voice_spectrum_last_reliability_kernel_ms(af_voice_spectrum *h, double *ms, int32_t capacity) {
  if (!h || !ms) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  if (capacity < 5) return fail(AF_ERR_INVALID_ARGUMENT, "ms must hold 5 values");
  std::fill(ms, ms + 5, 0.0);
  if (h->events.marks() == 0) return AF_OK;
  AF_HIP(hipSetDevice(h->device));
  AF_HIP(h->events.wait_last());
  for (size_t i = 0; i < h->span_kind.size() && 2 * i + 1 < h->events.marks(); ++i) {
    if (h->span_kind[i] < 0) continue;
    double span = 0.0;
    AF_HIP(h->events.elapsed(2 * i, 2 * i + 1, &span));
    ms[h->span_kind[i]] += span;
  }
  return AF_OK;
}

int af_voice_spectrum_last_kernel_ms(af_voice_spectrum *h, double *ms) {
  if (!h || !ms) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  *ms = 0.0;
  if (h->events.marks() == 0) return AF_OK;
  AF_HIP(hipSetDevice(h->device));
  AF_HIP(h->events.wait_last());
  for (size_t i = 0; i + 1 < h->events.marks(); i += 2) {
    double span = 0.0;
    AF_HIP(h->events.elapsed(i, i + 1, &span));
    *ms += span;
  }
  return AF_OK;
}

int af_voice_spectrum_smooth_rows(af_voice_spectrum *h, const double *rows_db, int32_t n_rows, double *out) {
  if (!h || !rows_db || !out) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  if (n_rows <= 0) return fail(AF_ERR_INVALID_ARGUMENT, "n_rows must be positive");
  AF_HIP(hipSetDevice(h->device));
  h->touched_device = true;
  if (int rc = vs_upload_tables(h)) return rc;
  const size_t K = (size_t)h->bins, P = af::kVsSmoothPasses, MB = af::kVsMaxBands, bytes = sizeof(double) * K * (size_t)n_rows;
  const int32_t *tb = h->d_bands;
  std::vector<int32_t> index((size_t)n_rows);
  for (int32_t i = 0; i < n_rows; ++i) index[(size_t)i] = i;
  AF_HIP(h->d_rows_db.reserve_exact(bytes));  // (every call synchronises before it returns: the per-tile scratch is free)
  AF_HIP(h->d_rows_smooth.reserve_exact(bytes));
  AF_HIP(h->d_smooth_rows.reserve_exact(sizeof(int32_t) * (size_t)n_rows));
  AF_HIP(hipMemcpy(h->d_rows_db, rows_db, bytes, hipMemcpyHostToDevice));
  AF_HIP(hipMemcpy(h->d_smooth_rows, index.data(), sizeof(int32_t) * (size_t)n_rows, hipMemcpyHostToDevice));
  AF_HIP(af::launch_vs_smooth(h->d_rows_db, h->d_smooth_rows, n_rows, (int32_t)K, tb, h->d_centre, tb + P, tb + P + P * MB,
                              tb + P + 2 * P * MB, tb + P + 2 * P * MB + K, h->d_freqs, h->d_rows_smooth, nullptr));
  AF_HIP(hipMemcpy(out, h->d_rows_smooth, bytes, hipMemcpyDeviceToHost));
  return AF_OK;
}

}  // extern "C"
