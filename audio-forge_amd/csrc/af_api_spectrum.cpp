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
  // the voiced frames' spectra of the last call that kept them
  bool have_windows = false;
  std::vector<int64_t> win_offset;  // [n_streams + 1] rows
  std::vector<double> win_raw, win_smooth, win_linear;
  ~af_voice_spectrum() {
    if (touched_device) { (void)hipSetDevice(device); (void)hipDeviceSynchronize(); }
  }
};

namespace {

double vs_percentile_sorted(const std::vector<double> &s, double q) {  // np.percentile, method "linear"
  const int n = (int)s.size();
  const double idx = (q / 100.0) * (double)(n - 1);
  const int lo = std::min(std::max((int)std::floor(idx), 0), n - 1), hi = std::min(lo + 1, n - 1);
  const double t = idx - (double)lo, a = s[(size_t)lo], b = s[(size_t)hi], diff = b - a;
  double r = a + diff * t;
  if (t >= 0.5) r = b - diff * (1.0 - t);
  return r;
}

double vs_median(std::vector<double> v) {  // np.median
  std::sort(v.begin(), v.end());
  const size_t n = v.size();
  return n % 2 ? v[n / 2] : (v[n / 2 - 1] + v[n / 2]) / 2.0;
}

double vs_interp(double x, const std::vector<double> &xp, const std::vector<double> &fp) {  // np.interp, ends held
  const int n = (int)xp.size();
  if (x < xp[0]) return fp[0];
  if (x >= xp[(size_t)n - 1]) return fp[(size_t)n - 1];
  int lo = 0, hi = n - 1;
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (x >= xp[(size_t)mid]) lo = mid; else hi = mid;
  }
  const double slope = (fp[(size_t)lo + 1] - fp[(size_t)lo]) / (xp[(size_t)lo + 1] - xp[(size_t)lo]);
  return slope * (x - xp[(size_t)lo]) + fp[(size_t)lo];
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
               VsDecision &d) {
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
    std::vector<double> xp((size_t)n_vad), fp((size_t)n_vad);
    const int64_t win = std::max<int64_t>(1, (int64_t)std::ceil((double)fs * (double)af::kVsSileroWindow / (double)af::kVsSileroRate));
    for (int64_t i = 0; i < n_vad; ++i) {
      xp[(size_t)i] = ((double)i + 0.5) * (double)win;
      fp[(size_t)i] = std::min(std::max(vad[i], 0.0), 1.0);
    }
    const double support = std::max(af::kVsRmsGateDb, floor_db + 0.25 * wide);
    std::vector<uint8_t> combined((size_t)F);
    int count = 0, active = 0;
    for (int f = 0; f < F; ++f) {
      const double centre = (double)((int64_t)f * hop) + (double)N * 0.5;
      const double post = vs_interp(centre, xp, fp);
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
  if (explicit_noise) {
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
  h->events.restart();
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
    vs_decide(&sums[(size_t)s * C * 2], F, N, h->sample_rate, vad ? vad + (int64_t)s * n_vad : nullptr, n_vad, explicit_noise, dec[(size_t)s]);
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
  const bool keep = out->keep_windows != 0;
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
  std::vector<int32_t> voiced_rows, first_row;
  for (int t0 = 0; t0 < B; t0 += tile) {
    const int t1 = std::min(B, t0 + tile);
    items.clear(); jobs.clear(); voiced_rows.clear(); first_row.clear();
    for (int s = t0; s < t1; ++s) {  // per stream: voiced frames | unvoiced frames (in-capture noise) | noise capture frames
      const VsDecision &d = dec[(size_t)s];
      const int32_t row0 = (int32_t)items.size();
      first_row.push_back(row0);
      for (int f = 0; f < F; ++f)
        if (d.mask[(size_t)f]) {
          voiced_rows.push_back((int32_t)items.size());
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
    const size_t R = items.size(), V = keep ? voiced_rows.size() : 0;
    medians.assign((size_t)(t1 - t0) * 2 * K, nan);
    if (R > 0) {
      AF_HIP(h->d_rows_linear.reserve_exact(row_bytes * R));
      if (keep) AF_HIP(h->d_rows_db.reserve_exact(row_bytes * R));
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
                                          (int32_t)R, N, h->d_window, h->d_twiddles, h->sumw2, keep ? h->d_rows_db.get() : nullptr,
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
      if (V > 0) {
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

}  // extern "C"
