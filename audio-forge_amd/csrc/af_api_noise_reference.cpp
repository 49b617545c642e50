// af_api_noise_reference.cpp -- the C ABI of the batched room-noise reference analysis (af_noise_reference_*):
// python/mic_eq/analysis/noise_reference.py:118-546.  The kernels do what is O(samples) and O(frames x bins); everything that is
// O(frames) or O(bins) per stream (percentiles, the VAD interpolation, the quiet-frame mask, spread / stability / flux, the
// thresholds and the scores) is decided here in f64, between the frame powers and the spectra and after the medians.
// Kernels and tables: af_noise_reference.hip / af_noise_reference_host.hpp; the column medians are af_spectrum.hip's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "af_api_internal.hpp"
#include "af_numpy_rules.h"
#include "af_noise_reference_host.hpp"
#include "af_spectrum_host.hpp"

struct af_noise_reference {
  int device = 0, frame = 0, bins = 0;
  uint32_t sample_rate = 0;
  bool touched_device = false;
  double sumw2 = 0.0;
  af::NrPlan plan = {};
  af::NrBandTable bands = {};
  std::vector<double> window, twiddles, freqs;
  af::DeviceBuffer<double> d_window, d_twiddles;  // uploaded at the first call
  af::DeviceBuffer<float> d_noise, d_speech;      // staging of the host entry point
  af::DeviceBuffer<af::NrSampleStats> d_stats;
  af::DeviceBuffer<double> d_noise_sums, d_speech_sums, d_noise_power, d_speech_power;
  af::DeviceBuffer<double> d_psd, d_band_power, d_medians;  // per tile of streams
  af::DeviceBuffer<af::NrFrameItem> d_items;
  af::DeviceBuffer<af::VsMedianJob> d_jobs;
  af::EventChain events;          // pairs of marks around the kernels of the last call
  std::vector<int8_t> span_kind;  // per pair: which of the four stages it times
  ~af_noise_reference() {
    if (touched_device) { (void)hipSetDevice(device); (void)hipDeviceSynchronize(); }
  }
};

namespace {

const double kNan = std::numeric_limits<double>::quiet_NaN();

double nr_percentile(std::vector<double> v, double q) {  // np.percentile, method "linear", with its two-sided lerp
  std::sort(v.begin(), v.end());
  return af_percentile_sorted(v.data(), (int)v.size(), q);  // the one restatement of the rule, af_numpy_rules.h
}

double nr_median(std::vector<double> v) {  // np.median
  std::sort(v.begin(), v.end());
  const size_t n = v.size();
  return n % 2 ? v[n / 2] : (v[n / 2 - 1] + v[n / 2]) / 2.0;
}

double nr_clip(double v, double lo, double hi) { return std::min(std::max(v, lo), hi); }

double nr_db(double power) { return 10.0 * std::log10(std::max(power, 1e-18)); }

double nr_interp(double x, const double *xp, const double *fp, int n) {  // np.interp, ends held
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

// _interpolate_vad, :188-205: posteriors spread evenly over the capture, at the frames' centres
bool nr_interpolate_vad(const double *vad, int64_t n_vad, int frames, std::vector<double> &out) {
  if (!vad || n_vad <= 0 || frames <= 0) return false;
  std::vector<double> xp((size_t)n_vad), fp((size_t)n_vad);
  for (int64_t i = 0; i < n_vad; ++i) {
    xp[(size_t)i] = ((double)i + 0.5) / (double)n_vad;
    fp[(size_t)i] = nr_clip(vad[i], 0.0, 1.0);
  }
  out.resize((size_t)frames);
  for (int f = 0; f < frames; ++f) out[(size_t)f] = nr_interp(((double)f + 0.5) / (double)frames, xp.data(), fp.data(), (int)n_vad);
  return true;
}

double nr_sum8(const double *a) { return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7])); }  // np.sum of 8 values

// what the host keeps per stream between the two groups of kernels
struct NrStream {
  std::vector<double> speech_rms;
  std::vector<int32_t> quiet;  // the voice frames _select_in_capture_noise keeps, :252-277
  int quiet_count = 0;         // its third return
  bool selected = false;
  double in_capture_rms_db = 0.0;
};

// _select_in_capture_noise up to its mask, from the voice capture's frame powers
void nr_select_quiet(const double *power, int F, const double *vad, int64_t n_vad, NrStream &st) {
  st.quiet.clear();
  st.quiet_count = 0;
  st.selected = false;
  st.speech_rms.resize((size_t)F);
  for (int f = 0; f < F; ++f) st.speech_rms[(size_t)f] = nr_db(power[f]);
  if (F < 4) return;
  const std::vector<double> &rms = st.speech_rms;
  std::vector<double> post;
  std::vector<int32_t> mask;
  if (nr_interpolate_vad(vad, n_vad, F, post)) {
    const double threshold = nr_percentile(rms, 35.0);
    for (int f = 0; f < F; ++f)
      if (post[(size_t)f] <= 0.25 && rms[(size_t)f] <= threshold) mask.push_back(f);
  } else {
    const double spread = nr_percentile(rms, 90.0) - nr_percentile(rms, 10.0);
    if (spread < 6.0) return;
    const double threshold = nr_percentile(rms, 15.0);
    for (int f = 0; f < F; ++f)
      if (rms[(size_t)f] <= threshold) mask.push_back(f);
  }
  st.quiet_count = (int)mask.size();
  const int minimum = std::max(3, (int)std::ceil((double)F * 0.05));
  if (st.quiet_count < minimum) return;
  st.selected = true;
  st.quiet = mask;
  std::vector<double> kept;
  for (int32_t f : mask) kept.push_back(rms[(size_t)f]);
  st.in_capture_rms_db = nr_median(kept);
}

// the dB median of a column from its two middle PSD values: np.median over 10 log10(max(., 1e-18)), which only selects
void nr_median_db(const double *middles /* [2][K] */, int K, double *out) {
  for (int k = 0; k < K; ++k) {
    const double lo = nr_db(middles[k]), hi = middles[K + k] == middles[k] ? lo : nr_db(middles[K + k]);
    out[k] = (lo + hi) / 2.0;
  }
}

// analyze_noise_reference from :299 on for one stream.  explicit_db / in_capture_db: the medians on the frame grid (in_capture_db
// null when none was selected); spectra out on `freqs` (the frame grid, or the grid of :339 below one frame).
void nr_decide(const af_noise_reference *h, int64_t n_noise, const af::NrSampleStats &ss, int Fn, const double *noise_power,
               const double *band_power /* [Fn][kNrBands] */, const double *noise_vad, int64_t n_noise_vad, const NrStream &st, int Fs,
               double age, uint32_t mismatch, const std::vector<double> &freqs, const double *explicit_db, const double *in_capture_db,
               af_noise_reference_row &r, double *explicit_out, double *conservative_out, double *in_capture_out, double *frame_rms_out,
               double *band_levels_out) {
  const int NB = h->bands.n_bands, K = (int)freqs.size(), KB = af::kNrBands;
  const double fs = (double)h->sample_rate, n = (double)n_noise;
  uint32_t reasons = 0, guidance = 0;
  bool invalid = false, questionable = false;
  const double finite_fraction = n_noise ? (double)ss.finite / n : 0.0;
  const double duration_s = n / fs;
  const double noise_rms_db = nr_db(n_noise ? ss.sum_squares / n : 0.0);
  const double noise_peak_db = 20.0 * std::log10(std::max(n_noise ? ss.peak : 0.0, 1e-9));
  const double crest_factor_db = std::max(0.0, noise_peak_db - noise_rms_db);
  const double clipped_fraction = n_noise ? (double)ss.clipped / n : 0.0;
  const double zero_fraction = n_noise ? (double)ss.zero / n : 1.0;

  if (duration_s < af::kNrMinDurationS) { invalid = true; reasons |= AF_NOISE_REASON_TOO_SHORT; guidance |= 1u << 0; }
  if (finite_fraction < 1.0) { invalid = true; reasons |= AF_NOISE_REASON_NON_FINITE; guidance |= 1u << 1; }
  if (noise_rms_db <= -95.0 || (zero_fraction >= 0.995 && noise_peak_db <= -90.0)) {
    invalid = true; reasons |= AF_NOISE_REASON_SILENT; guidance |= 1u << 2;
  }
  if (clipped_fraction > 0.001) { invalid = true; reasons |= AF_NOISE_REASON_CLIPPED; guidance |= 1u << 3; }
  else if (clipped_fraction > 0.0) { questionable = true; reasons |= AF_NOISE_REASON_ISOLATED_CLIPS; guidance |= 1u << 4; }

  double rms_spread_db = 120.0, octave_stability_db = 120.0, spectral_flux_db = 120.0;
  std::vector<double> frame_rms((size_t)Fn);
  if (Fn == 0) {  // :336-343
    invalid = true;
    reasons |= AF_NOISE_REASON_TOO_FEW_WINDOWS;
    for (int k = 0; k < K; ++k) explicit_out[k] = -120.0;
  } else {
    std::memcpy(explicit_out, explicit_db, sizeof(double) * (size_t)K);
    for (int f = 0; f < Fn; ++f) frame_rms[(size_t)f] = nr_db(noise_power[f]);
    rms_spread_db = nr_percentile(frame_rms, 90.0) - nr_percentile(frame_rms, 10.0);  // :152-154
    octave_stability_db = 0.0;
    spectral_flux_db = 0.0;
    if (NB > 0) {  // :155-171
      std::vector<double> levels((size_t)Fn * NB), column((size_t)Fn), spread((size_t)NB), row((size_t)NB);
      for (int f = 0; f < Fn; ++f)
        for (int b = 0; b < NB; ++b) levels[(size_t)f * NB + b] = nr_db(band_power[(size_t)f * KB + b]);
      for (int b = 0; b < NB; ++b) {
        for (int f = 0; f < Fn; ++f) column[(size_t)f] = levels[(size_t)f * NB + b];
        spread[(size_t)b] = nr_percentile(column, 90.0) - nr_percentile(column, 10.0);
      }
      octave_stability_db = nr_median(spread);
      if (Fn >= 2) {
        std::vector<double> normalized((size_t)Fn * NB), flux((size_t)Fn - 1);
        for (int f = 0; f < Fn; ++f) {
          std::copy(&levels[(size_t)f * NB], &levels[(size_t)f * NB] + NB, row.begin());
          const double mid = nr_median(row);
          for (int b = 0; b < NB; ++b) normalized[(size_t)f * NB + b] = levels[(size_t)f * NB + b] - mid;
        }
        for (int f = 0; f + 1 < Fn; ++f) {
          for (int b = 0; b < NB; ++b) row[(size_t)b] = std::fabs(normalized[(size_t)(f + 1) * NB + b] - normalized[(size_t)f * NB + b]);
          flux[(size_t)f] = nr_median(row);
        }
        spectral_flux_db = nr_percentile(flux, 95.0);
      }
      if (band_levels_out)
        for (int f = 0; f < Fn; ++f)
          for (int b = 0; b < KB; ++b) band_levels_out[(size_t)f * KB + b] = b < NB ? levels[(size_t)f * NB + b] : kNan;
    } else if (band_levels_out) {
      std::fill(band_levels_out, band_levels_out + (size_t)Fn * KB, kNan);
    }
    if (frame_rms_out) std::copy(frame_rms.begin(), frame_rms.end(), frame_rms_out);
    if (rms_spread_db > 12.0 || octave_stability_db > 14.0) { invalid = true; reasons |= AF_NOISE_REASON_CHANGING_EVENTS; guidance |= 1u << 5; }
    else if (rms_spread_db > 6.0 || octave_stability_db > 8.0) { questionable = true; reasons |= AF_NOISE_REASON_NOT_STATIONARY; guidance |= 1u << 6; }
    if (spectral_flux_db > 10.0) { invalid = true; reasons |= AF_NOISE_REASON_DOMINANT_TRANSIENTS; guidance |= 1u << 7; }
    else if (spectral_flux_db > 6.0 || crest_factor_db > 24.0) { questionable = true; reasons |= AF_NOISE_REASON_STRONG_TRANSIENTS; guidance |= 1u << 7; }
  }

  double vad_ratio = 0.0, vad_p90 = 0.0;  // :367-388
  std::vector<double> post;
  if (nr_interpolate_vad(noise_vad, n_noise_vad, Fn, post)) {
    int above = 0;
    for (double p : post) above += p >= af::kNrVadContamination;
    vad_ratio = (double)above / (double)Fn;
    vad_p90 = nr_percentile(post, 90.0);
  }
  if (vad_ratio > 0.30) { invalid = true; reasons |= AF_NOISE_REASON_SPEECH_PRESENT; guidance |= 1u << 8; }
  else if (vad_ratio > 0.08 || vad_p90 > 0.55) { questionable = true; reasons |= AF_NOISE_REASON_POSSIBLE_SPEECH; guidance |= 1u << 9; }

  if (mismatch & 0x3fu) { invalid = true; reasons |= (mismatch & 0x3fu) * AF_NOISE_REASON_METADATA; guidance |= 1u << 10; }  // :397-400
  const bool have_age = !std::isnan(age);
  const double capture_age_s = have_age ? std::max(0.0, age) : kNan;
  if (have_age) {
    if (capture_age_s > af::kNrInvalidAgeS) { invalid = true; reasons |= AF_NOISE_REASON_STALE; guidance |= 1u << 11; }
    else if (capture_age_s > af::kNrQuestionableAgeS) { questionable = true; reasons |= AF_NOISE_REASON_MAY_BE_STALE; guidance |= 1u << 12; }
  }

  double level_delta_db = kNan, shape_distance_db = kNan, conservative_rms_db = noise_rms_db;  // :422-470
  std::memcpy(conservative_out, explicit_out, sizeof(double) * (size_t)K);
  const bool have_in_capture = st.selected && in_capture_db;
  if (have_in_capture) {
    if (Fn > 0) std::memcpy(in_capture_out, in_capture_db, sizeof(double) * (size_t)K);  // the same grid: np.interp returns its knots
    else
      for (int k = 0; k < K; ++k) in_capture_out[k] = nr_interp(freqs[(size_t)k], h->freqs.data(), in_capture_db, h->bins);
    level_delta_db = st.in_capture_rms_db - noise_rms_db;
    bool any = false;
    for (int k = 0; k < K; ++k) any = any || (freqs[(size_t)k] >= 80.0 && freqs[(size_t)k] <= 8000.0);
    std::vector<double> e, c;
    for (int k = 0; k < K; ++k)
      if (!any || (freqs[(size_t)k] >= 80.0 && freqs[(size_t)k] <= 8000.0)) { e.push_back(explicit_out[k]); c.push_back(in_capture_out[k]); }
    const double me = nr_median(e), mc = nr_median(c);
    for (size_t i = 0; i < e.size(); ++i) e[i] = std::fabs((e[i] - me) - (c[i] - mc));
    shape_distance_db = nr_median(e);
    for (int k = 0; k < K; ++k) conservative_out[k] = std::max(explicit_out[k], in_capture_out[k]);
    conservative_rms_db = std::max(noise_rms_db, st.in_capture_rms_db);
    if (level_delta_db > 12.0 || shape_distance_db > 10.0) { invalid = true; reasons |= AF_NOISE_REASON_MISMATCH; guidance |= 1u << 13; }
    else if (level_delta_db > 6.0 || shape_distance_db > 5.5) { questionable = true; reasons |= AF_NOISE_REASON_PARTIAL_MATCH; guidance |= 1u << 14; }
    else if (level_delta_db < -20.0) { invalid = true; reasons |= AF_NOISE_REASON_LEVEL_CHANGED; guidance |= 1u << 15; }
    else if (level_delta_db < -12.0) { questionable = true; reasons |= AF_NOISE_REASON_MUCH_LOUDER; guidance |= 1u << 16; }
  } else {
    std::fill(in_capture_out, in_capture_out + K, kNan);
  }

  double consistency = 1.0;  // :472-509
  if (have_in_capture) {
    consistency *= nr_clip(1.0 - std::max(0.0, level_delta_db) / 12.0, 0.0, 1.0);
    consistency *= nr_clip(1.0 - shape_distance_db / 10.0, 0.0, 1.0);
  }
  const double values[8] = {nr_clip(duration_s / 3.0, 0.0, 1.0),
                            nr_clip((finite_fraction - 0.995) / 0.005, 0.0, 1.0),
                            nr_clip(1.0 - rms_spread_db / 12.0, 0.0, 1.0),
                            nr_clip(1.0 - octave_stability_db / 14.0, 0.0, 1.0),
                            nr_clip(1.0 - std::max(0.0, crest_factor_db - 12.0) / 18.0, 0.0, 1.0),
                            nr_clip(1.0 - vad_ratio / 0.30, 0.0, 1.0),
                            consistency,
                            have_age ? nr_clip(1.0 - capture_age_s / af::kNrInvalidAgeS, 0.0, 1.0) : 1.0};
  double weights[8] = {0.10, 0.10, 0.18, 0.15, 0.10, 0.15, 0.17, 0.05}, terms[8];
  const double total = nr_sum8(weights);
  for (int i = 0; i < 8; ++i) {
    weights[i] /= total;
    terms[i] = weights[i] * std::log(std::max(nr_clip(values[i], 0.0, 1.0), 0.02));
  }
  double quality = std::exp(nr_sum8(terms));
  if (invalid) quality = std::min(quality, 0.20);
  else if (questionable) quality = std::min(quality, 0.64);

  r = af_noise_reference_row{};
  r.status = invalid ? AF_NOISE_STATUS_INVALID : (questionable ? AF_NOISE_STATUS_QUESTIONABLE : AF_NOISE_STATUS_USABLE);
  r.conservative = questionable || invalid || have_in_capture;
  r.reasons = reasons;
  r.guidance = guidance;
  r.quality_score = nr_clip(quality, 0.0, 1.0);
  r.duration_s = duration_s;
  r.finite_fraction = finite_fraction;
  r.noise_rms_db = noise_rms_db;
  r.conservative_noise_rms_db = conservative_rms_db;
  r.noise_peak_db = noise_peak_db;
  r.crest_factor_db = crest_factor_db;
  r.clipped_fraction = clipped_fraction;
  r.zero_fraction = zero_fraction;
  r.rms_spread_db = rms_spread_db;
  r.octave_stability_db = octave_stability_db;
  r.spectral_flux_db = spectral_flux_db;
  r.vad_contamination_ratio = vad_ratio;
  r.vad_contamination_p90 = vad_p90;
  r.capture_age_s = capture_age_s;
  r.in_capture_level_delta_db = level_delta_db;
  r.spectral_shape_distance_db = shape_distance_db;
  r.noise_sum_squares = ss.sum_squares;
  r.noise_peak = ss.peak;
  r.finite_samples = ss.finite;
  r.clipped_samples = ss.clipped;
  r.zero_samples = ss.zero;
  r.in_capture_noise_frame_count = st.quiet_count;
  r.noise_frames = Fn;
  r.speech_frames = Fs;
  r.n_bands = NB;
  r.has_in_capture_spectrum = have_in_capture;
}

int nr_upload_tables(af_noise_reference *h) {
  if (h->d_window) return AF_OK;
  AF_HIP(h->d_twiddles.reserve_exact(sizeof(double) * h->twiddles.size()));
  AF_HIP(hipMemcpy(h->d_twiddles, h->twiddles.data(), sizeof(double) * h->twiddles.size(), hipMemcpyHostToDevice));
  AF_HIP(h->d_window.reserve_exact(sizeof(double) * h->window.size()));  // last: its presence means "all tables are up"
  AF_HIP(h->d_window.keep_if(hipMemcpy(h->d_window, h->window.data(), sizeof(double) * h->window.size(), hipMemcpyHostToDevice)));
  return AF_OK;
}

int64_t nr_frames(const af_noise_reference *h, int64_t n) { return n < h->frame ? 0 : (n - h->frame) / (h->frame / 2) + 1; }

// every argument check of the two entry points; no HIP call
int nr_check(af_noise_reference *h, const float *noise, int64_t n_noise, int32_t n_streams, int64_t noise_stride, const float *speech,
             int64_t n_speech, int64_t speech_stride, const double *noise_vad, int64_t n_noise_vad, const double *speech_vad,
             int64_t n_speech_vad, const af_noise_reference_outputs *out) {
  if (!h) return fail(AF_ERR_INVALID_ARGUMENT, "noise reference handle is null");
  if (!out) return fail(AF_ERR_INVALID_ARGUMENT, "outputs is null");
  if (n_streams <= 0) return fail(AF_ERR_INVALID_ARGUMENT, "n_streams must be positive");
  if (n_noise < 0 || noise_stride < n_noise) return fail(AF_ERR_INVALID_ARGUMENT, "noise_stride must cover n_noise >= 0");
  if (!noise && n_noise > 0) return fail(AF_ERR_INVALID_ARGUMENT, "noise is null");
  if (speech && (n_speech < 0 || speech_stride < n_speech)) return fail(AF_ERR_INVALID_ARGUMENT, "speech_stride must cover n_speech >= 0");
  if (!speech && n_speech > 0) return fail(AF_ERR_INVALID_ARGUMENT, "n_speech without speech");
  if ((noise_vad != nullptr) != (n_noise_vad > 0) || n_noise_vad < 0)
    return fail(AF_ERR_INVALID_ARGUMENT, "noise_vad and a positive n_noise_vad go together");
  if ((speech_vad != nullptr) != (n_speech_vad > 0) || n_speech_vad < 0)
    return fail(AF_ERR_INVALID_ARGUMENT, "speech_vad and a positive n_speech_vad go together");
  if (nr_frames(h, n_noise) > (1 << 22) || nr_frames(h, n_speech) > (1 << 22))
    return fail(AF_ERR_UNSUPPORTED, "more than 2^22 frames per stream");
  return AF_OK;
}

int nr_analyze(af_noise_reference *h, const float *d_noise, int64_t n_noise, int32_t B, int64_t noise_stride, const float *d_speech,
               int64_t n_speech, int64_t speech_stride, const double *noise_vad, int64_t n_noise_vad, const double *speech_vad,
               int64_t n_speech_vad, const double *ages, const uint32_t *mismatch, const af_noise_reference_outputs *out) {
  const int N = h->frame, hop = N / 2, K = h->bins, KB = af::kNrBands;
  const int Fn = (int)nr_frames(h, n_noise), Cn = Fn ? Fn + 1 : 0;
  const int Fs = d_speech ? (int)nr_frames(h, n_speech) : 0, Cs = Fs ? Fs + 1 : 0;
  std::vector<double> grid;  // the grid of the spectra returned: the frames', or :339's below one frame
  if (Fn) grid = h->freqs; else af::nr_freqs(h->sample_rate, (int)std::max<int64_t>(2, n_noise), grid);
  const int Ko = (int)grid.size();
  hipStream_t q = nullptr;
  h->events.restart();
  h->span_kind.clear();
  const auto span = [&](int8_t kind) { h->span_kind.push_back(kind); return h->events.mark(q); };
  if (int rc = nr_upload_tables(h)) return rc;

  // 1. sample statistics, chunk sums and centred frame powers
  std::vector<af::NrSampleStats> stats((size_t)B);
  std::vector<double> nsums((size_t)B * Cn * 2), npower((size_t)B * Fn), spower((size_t)B * Fs);
  AF_HIP(h->d_stats.reserve_exact(sizeof(af::NrSampleStats) * (size_t)B));
  AF_HIP(h->d_noise_sums.reserve_exact(sizeof(double) * std::max<size_t>(1, nsums.size())));
  AF_HIP(h->d_speech_sums.reserve_exact(sizeof(double) * std::max<size_t>(1, (size_t)B * Cs * 2)));
  AF_HIP(h->d_noise_power.reserve_exact(sizeof(double) * std::max<size_t>(1, npower.size())));
  AF_HIP(h->d_speech_power.reserve_exact(sizeof(double) * std::max<size_t>(1, spower.size())));
  AF_HIP(span(0));
  AF_HIP(af::launch_nr_sample_stats(d_noise, noise_stride, n_noise, B, h->d_stats, q));
  AF_HIP(af::launch_nr_chunk_sums(d_noise, noise_stride, B, Cn, hop, h->d_noise_sums, q));
  AF_HIP(af::launch_nr_chunk_sums(d_speech, speech_stride, B, Cs, hop, h->d_speech_sums, q));
  AF_HIP(h->events.mark(q));
  AF_HIP(span(1));
  AF_HIP(af::launch_nr_frame_power(d_noise, noise_stride, h->d_noise_sums, B, Fn, hop, h->d_noise_power, q));
  AF_HIP(af::launch_nr_frame_power(d_speech, speech_stride, h->d_speech_sums, B, Fs, hop, h->d_speech_power, q));
  AF_HIP(h->events.mark(q));
  AF_HIP(hipMemcpy(stats.data(), h->d_stats, sizeof(af::NrSampleStats) * (size_t)B, hipMemcpyDeviceToHost));
  if (!nsums.empty()) AF_HIP(hipMemcpy(nsums.data(), h->d_noise_sums, sizeof(double) * nsums.size(), hipMemcpyDeviceToHost));
  if (!npower.empty()) AF_HIP(hipMemcpy(npower.data(), h->d_noise_power, sizeof(double) * npower.size(), hipMemcpyDeviceToHost));
  if (!spower.empty()) AF_HIP(hipMemcpy(spower.data(), h->d_speech_power, sizeof(double) * spower.size(), hipMemcpyDeviceToHost));

  // 2. the quiet frames of every voice capture
  std::vector<NrStream> streams((size_t)B);
  int64_t max_rows = Fn;
  for (int s = 0; s < B; ++s) {
    nr_select_quiet(Fs ? &spower[(size_t)s * Fs] : nullptr, Fs, speech_vad ? speech_vad + (int64_t)s * n_speech_vad : nullptr, n_speech_vad,
                    streams[(size_t)s]);
    max_rows = std::max<int64_t>(max_rows, Fn + (int64_t)streams[(size_t)s].quiet.size());
  }

  // 3. frame spectra, band sums and medians, a tile of streams at a time; then the verdicts
  const size_t row_bytes = sizeof(double) * (size_t)K;
  const int64_t budget_rows = std::max<int64_t>(1, ((int64_t)256 << 20) / (int64_t)row_bytes);
  const int tile = (int)std::min<int64_t>(af::kNrTileStreams, std::max<int64_t>(1, budget_rows / std::max<int64_t>(1, max_rows)));
  std::vector<af::NrFrameItem> items;
  std::vector<af::VsMedianJob> jobs;
  std::vector<int32_t> first_row;
  std::vector<double> middles, band_power, explicit_db((size_t)K), in_capture_db((size_t)K);
  std::vector<double> spectra((size_t)3 * Ko);
  for (int t0 = 0; t0 < B; t0 += tile) {
    const int t1 = std::min(B, t0 + tile), T = t1 - t0;
    items.clear(); jobs.clear(); first_row.clear();
    for (int s = t0; s < t1; ++s) {  // per stream: the noise frames | the quiet voice frames
      const int32_t row0 = (int32_t)items.size();
      first_row.push_back(row0);
      for (int f = 0; f < Fn; ++f) items.push_back({0, s, f, (int32_t)items.size()});
      if (Fn) jobs.push_back({row0, Fn, 2 * (s - t0), 0});
      const std::vector<int32_t> &quiet = streams[(size_t)s].quiet;
      const int32_t r = (int32_t)items.size();
      for (int32_t f : quiet) items.push_back({1, s, f, (int32_t)items.size()});
      if (!quiet.empty()) jobs.push_back({r, (int32_t)quiet.size(), 2 * (s - t0) + 1, 0});
    }
    const size_t R = items.size();
    middles.assign((size_t)T * 4 * K, kNan);  // [stream][noise | quiet][lower | upper][K]
    band_power.assign(R * KB, 0.0);
    if (R > 0) {
      AF_HIP(h->d_psd.reserve_exact(row_bytes * R));
      AF_HIP(h->d_band_power.reserve_exact(sizeof(double) * KB * R));
      AF_HIP(h->d_items.reserve_exact(sizeof(af::NrFrameItem) * R));
      AF_HIP(h->d_jobs.reserve_exact(sizeof(af::VsMedianJob) * jobs.size()));
      AF_HIP(h->d_medians.reserve_exact(row_bytes * 4 * (size_t)T));
      AF_HIP(hipMemcpy(h->d_items, items.data(), sizeof(af::NrFrameItem) * R, hipMemcpyHostToDevice));
      AF_HIP(hipMemcpy(h->d_jobs, jobs.data(), sizeof(af::VsMedianJob) * jobs.size(), hipMemcpyHostToDevice));
      AF_HIP(span(2));
      AF_HIP(af::launch_nr_frame_spectra(d_noise, noise_stride, h->d_noise_sums, Cn, d_speech, speech_stride, h->d_speech_sums, Cs,
                                         h->d_items, (int32_t)R, N, h->plan, h->bands, h->d_window, h->d_twiddles, h->sumw2, h->d_psd,
                                         h->d_band_power, q));
      AF_HIP(h->events.mark(q));
      AF_HIP(span(3));
      AF_HIP(af::launch_vs_median(h->d_psd, h->d_jobs, (int32_t)jobs.size(), K, h->d_medians, q));
      AF_HIP(h->events.mark(q));
      AF_HIP(hipMemcpy(band_power.data(), h->d_band_power, sizeof(double) * KB * R, hipMemcpyDeviceToHost));
      AF_HIP(hipMemcpy(middles.data(), h->d_medians, row_bytes * 4 * (size_t)T, hipMemcpyDeviceToHost));  // one copy a tile
      std::vector<uint8_t> wrote((size_t)2 * T, 0);
      for (const af::VsMedianJob &j : jobs) wrote[(size_t)j.out] = 1;
      for (size_t o = 0; o < wrote.size(); ++o)  // rows no job wrote are NaN
        if (!wrote[o]) std::fill(&middles[o * 2 * K], &middles[o * 2 * K] + 2 * K, kNan);
      if (out->noise_psd && Fn)
        for (int s = t0; s < t1; ++s)
          AF_HIP(hipMemcpy(out->noise_psd + (size_t)s * Fn * K, h->d_psd + (size_t)first_row[(size_t)(s - t0)] * K, row_bytes * Fn,
                           hipMemcpyDeviceToHost));
    }
    for (int s = t0; s < t1; ++s) {
      const NrStream &st = streams[(size_t)s];
      const double *mid = &middles[(size_t)(s - t0) * 4 * K];
      if (Fn) nr_median_db(mid, K, explicit_db.data());
      if (st.selected) nr_median_db(mid + 2 * K, K, in_capture_db.data());
      af_noise_reference_row row;
      nr_decide(h, n_noise, stats[(size_t)s], Fn, Fn ? &npower[(size_t)s * Fn] : nullptr,
                band_power.data() + (size_t)first_row[(size_t)(s - t0)] * KB, noise_vad ? noise_vad + (int64_t)s * n_noise_vad : nullptr,
                n_noise_vad, st, Fs, ages ? ages[s] : kNan, mismatch ? mismatch[s] : 0u, grid, explicit_db.data(),
                st.selected ? in_capture_db.data() : nullptr, row, &spectra[0], &spectra[(size_t)Ko], &spectra[(size_t)2 * Ko],
                out->frame_rms_db ? out->frame_rms_db + (size_t)s * Fn : nullptr,
                out->band_levels_db ? out->band_levels_db + (size_t)s * Fn * KB : nullptr);
      if (out->rows) out->rows[s] = row;
      const size_t bytes = sizeof(double) * (size_t)Ko;
      if (out->explicit_spectrum_db) std::memcpy(out->explicit_spectrum_db + (size_t)s * Ko, &spectra[0], bytes);
      if (out->conservative_spectrum_db) std::memcpy(out->conservative_spectrum_db + (size_t)s * Ko, &spectra[(size_t)Ko], bytes);
      if (out->in_capture_spectrum_db) std::memcpy(out->in_capture_spectrum_db + (size_t)s * Ko, &spectra[(size_t)2 * Ko], bytes);
      if (out->band_power && Fn)
        std::memcpy(out->band_power + (size_t)s * Fn * KB, band_power.data() + (size_t)first_row[(size_t)(s - t0)] * KB, sizeof(double) * KB * Fn);
      if (out->explicit_middles) std::memcpy(out->explicit_middles + (size_t)s * 2 * K, mid, row_bytes * 2);
      if (out->in_capture_middles) std::memcpy(out->in_capture_middles + (size_t)s * 2 * K, mid + 2 * K, row_bytes * 2);
    }
  }
  AF_HIP(hipStreamSynchronize(q));
  if (out->noise_chunk_sums && !nsums.empty()) std::memcpy(out->noise_chunk_sums, nsums.data(), sizeof(double) * nsums.size());
  if (out->noise_frame_power && !npower.empty()) std::memcpy(out->noise_frame_power, npower.data(), sizeof(double) * npower.size());
  if (out->speech_frame_power && !spower.empty()) std::memcpy(out->speech_frame_power, spower.data(), sizeof(double) * spower.size());
  return AF_OK;
}

}  // namespace

extern "C" {

int af_noise_reference_create(uint32_t sample_rate, int32_t device, af_noise_reference **out) {
  if (!out) return fail(AF_ERR_INVALID_ARGUMENT, "out is null");
  *out = nullptr;
  if (sample_rate == 0) return fail(AF_ERR_INVALID_ARGUMENT, "sample_rate must be positive");
  if (device < 0) return fail(AF_ERR_INVALID_ARGUMENT, "device must be >= 0");
  if (sample_rate > 1000000u) return fail(AF_ERR_UNSUPPORTED, "sample rate %u Hz: the analysis frame does not fit the transform", sample_rate);
  const int N = af::nr_frame_size(sample_rate);
  af::NrPlan plan;
  if (N % 2 != 0)
    return fail(AF_ERR_UNSUPPORTED, "sample rate %u Hz: the analysis frame of %d samples is odd; the transform takes even frames", sample_rate, N);
  if (!af::nr_make_plan(N / 2, plan))
    return fail(AF_ERR_UNSUPPORTED, "sample rate %u Hz: half the analysis frame of %d samples has a prime factor above 7", sample_rate, N);
  if (N / 2 > af::kNrMaxHalf)
    return fail(AF_ERR_UNSUPPORTED, "sample rate %u Hz: the analysis frame of %d samples does not fit 160 KB of LDS (at most %d)",
                sample_rate, N, 2 * af::kNrMaxHalf);
  af_noise_reference *h = new af_noise_reference();
  h->device = device;
  h->sample_rate = sample_rate;
  h->frame = N;
  h->bins = N / 2 + 1;
  h->plan = plan;
  af::nr_make_window(N, h->window, &h->sumw2);
  af::nr_make_twiddles(N, h->twiddles);
  af::nr_freqs(sample_rate, N, h->freqs);
  af::nr_make_bands(sample_rate, h->freqs, h->bands);
  *out = h;
  return AF_OK;
}

void af_noise_reference_destroy(af_noise_reference *h) { delete h; }

int32_t af_noise_reference_frame_size(const af_noise_reference *h) { return h ? h->frame : 0; }

int32_t af_noise_reference_bins(const af_noise_reference *h, int64_t n_noise) {
  if (!h) return 0;
  return n_noise >= h->frame ? h->bins : (int32_t)(std::max<int64_t>(2, n_noise) / 2 + 1);
}

int64_t af_noise_reference_frames(const af_noise_reference *h, int64_t n_samples) { return h ? nr_frames(h, n_samples) : 0; }

int af_noise_reference_analyze_device(af_noise_reference *h, const float *d_noise, int64_t n_noise, int32_t n_streams, int64_t noise_stride,
                                      const float *d_speech, int64_t n_speech, int64_t speech_stride, const double *noise_vad,
                                      int64_t n_noise_vad, const double *speech_vad, int64_t n_speech_vad, const double *capture_age_s,
                                      const uint32_t *metadata_mismatch, const af_noise_reference_outputs *out) {
  if (int rc = nr_check(h, d_noise, n_noise, n_streams, noise_stride, d_speech, n_speech, speech_stride, noise_vad, n_noise_vad,
                        speech_vad, n_speech_vad, out))
    return rc;
  AF_HIP(hipSetDevice(h->device));
  h->touched_device = true;
  return nr_analyze(h, d_noise, n_noise, n_streams, noise_stride, d_speech, d_speech ? n_speech : 0, speech_stride, noise_vad,
                    n_noise_vad, speech_vad, n_speech_vad, capture_age_s, metadata_mismatch, out);
}

int af_noise_reference_analyze_host(af_noise_reference *h, const float *noise, int64_t n_noise, int32_t n_streams, int64_t noise_stride,
                                    const float *speech, int64_t n_speech, int64_t speech_stride, const double *noise_vad,
                                    int64_t n_noise_vad, const double *speech_vad, int64_t n_speech_vad, const double *capture_age_s,
                                    const uint32_t *metadata_mismatch, const af_noise_reference_outputs *out) {
  if (int rc = nr_check(h, noise, n_noise, n_streams, noise_stride, speech, n_speech, speech_stride, noise_vad, n_noise_vad, speech_vad,
                        n_speech_vad, out))
    return rc;
  AF_HIP(hipSetDevice(h->device));
  h->touched_device = true;
  const size_t f4 = sizeof(float);
  const bool with_speech = speech && n_speech > 0;
  AF_HIP(h->d_noise.reserve_exact(std::max<size_t>(f4, f4 * (size_t)n_streams * n_noise)));  // (every call synchronises before it returns)
  if (n_noise > 0)
    AF_HIP(hipMemcpy2D(h->d_noise, f4 * n_noise, noise, f4 * noise_stride, f4 * n_noise, n_streams, hipMemcpyHostToDevice));
  if (with_speech) {
    AF_HIP(h->d_speech.reserve_exact(f4 * (size_t)n_streams * n_speech));
    AF_HIP(hipMemcpy2D(h->d_speech, f4 * n_speech, speech, f4 * speech_stride, f4 * n_speech, n_streams, hipMemcpyHostToDevice));
  }
  return nr_analyze(h, h->d_noise, n_noise, n_streams, n_noise, with_speech ? h->d_speech.get() : nullptr, with_speech ? n_speech : 0,
                    n_speech, noise_vad, n_noise_vad, speech_vad, n_speech_vad, capture_age_s, metadata_mismatch, out);
}

int af_noise_reference_last_kernel_ms(af_noise_reference *h, double *ms, int32_t capacity) {
  if (!h || !ms) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  if (capacity < 4) return fail(AF_ERR_INVALID_ARGUMENT, "ms must hold 4 values");
  std::fill(ms, ms + 4, 0.0);
  if (h->events.marks() == 0) return AF_OK;
  AF_HIP(hipSetDevice(h->device));
  AF_HIP(h->events.wait_last());
  for (size_t i = 0; i < h->span_kind.size() && 2 * i + 1 < h->events.marks(); ++i) {
    double span = 0.0;
    AF_HIP(h->events.elapsed(2 * i, 2 * i + 1, &span));
    ms[h->span_kind[i]] += span;
  }
  return AF_OK;
}

}  // extern "C"
