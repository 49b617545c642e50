// af_api_speech_features.cpp -- the C ABI of the batched speech-feature measurement (af_speech_features_*):
// python/mic_eq/analysis/voice_setup.py:161-458.  The kernels do what is O(samples) and O(frames x bins); what is O(frames) per
// stream (frame levels, the adaptive floor, the VAD-fused mask, the loudness windows, the frame features and the frame model)
// is af_speech_features_math.h's, in f64, between the kernels.  Kernels and tables: af_speech_features.hip /
// af_speech_features_host.hpp; the medians over frames are af_spectrum.hip's.  The object and its analysis (af::sf_*,
// af_speech_features_impl.hpp) also serve af_device_rate_features_*, whose rates resample to 48 kHz in front of the K-weighting.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "af_speech_features_impl.hpp"

namespace {

int sf_upload_tables(af_speech_features *h) {
  if (h->d_window) return AF_OK;
  if (!h->phase_table.empty()) {
    AF_HIP(h->d_phase_table.reserve_exact(sizeof(double) * h->phase_table.size()));
    AF_HIP(hipMemcpy(h->d_phase_table, h->phase_table.data(), sizeof(double) * h->phase_table.size(), hipMemcpyHostToDevice));
  }
  AF_HIP(h->d_twiddles.reserve_exact(sizeof(double) * h->twiddles.size()));
  AF_HIP(hipMemcpy(h->d_twiddles, h->twiddles.data(), sizeof(double) * h->twiddles.size(), hipMemcpyHostToDevice));
  AF_HIP(h->d_window.reserve_exact(sizeof(double) * h->window.size()));  // last: its presence means "all tables are up"
  AF_HIP(h->d_window.keep_if(hipMemcpy(h->d_window, h->window.data(), sizeof(double) * h->window.size(), hipMemcpyHostToDevice)));
  return AF_OK;
}

// every argument check of the two entry points; no HIP call
int sf_check(af_speech_features *h, const float *speech, int64_t n, int32_t B, int64_t stride, const double *noise_rms_db,
             const double *vad, int64_t n_vad, const float *noise, int64_t m, int64_t noise_stride, const af_speech_features_outputs *out) {
  if (!h) return fail(AF_ERR_INVALID_ARGUMENT, "speech features handle is null");
  if (!out) return fail(AF_ERR_INVALID_ARGUMENT, "outputs is null");
  if (!speech) return fail(AF_ERR_INVALID_ARGUMENT, "speech is null");
  if (!noise_rms_db) return fail(AF_ERR_INVALID_ARGUMENT, "noise_rms_db is null");
  if (B <= 0) return fail(AF_ERR_INVALID_ARGUMENT, "n_streams must be positive");
  if (B > h->max_streams) return fail(AF_ERR_INVALID_ARGUMENT, "n_streams %d is above the handle's max_streams %d", B, h->max_streams);
  if (n < h->geo.frame)
    return fail(AF_ERR_INVALID_ARGUMENT, "speech capture of %lld samples is shorter than one analysis frame of %d", (long long)n,
                h->geo.frame);
  if (n > h->max_speech)
    return fail(AF_ERR_INVALID_ARGUMENT, "n_speech %lld is above the handle's max_speech_samples %lld", (long long)n, (long long)h->max_speech);
  if (stride < n) return fail(AF_ERR_INVALID_ARGUMENT, "speech_stride must cover n_speech");
  if ((vad != nullptr) != (n_vad > 0) || n_vad < 0)
    return fail(AF_ERR_INVALID_ARGUMENT, "vad_probabilities and a positive n_vad go together");
  if (noise && (m < 0 || noise_stride < m)) return fail(AF_ERR_INVALID_ARGUMENT, "noise_stride must cover n_noise >= 0");
  if (!noise && m > 0) return fail(AF_ERR_INVALID_ARGUMENT, "n_noise without noise");
  if (m > h->max_noise)
    return fail(AF_ERR_INVALID_ARGUMENT, "n_noise %lld is above the handle's max_noise_samples %lld", (long long)m, (long long)h->max_noise);
  if (sfm_frames_at(&h->geo, n) > (1 << 22) || sfm_frames_at(&h->geo, m) > (1 << 22))
    return fail(AF_ERR_UNSUPPORTED, "more than 2^22 frames per stream");
  return AF_OK;
}

bool all_finite(const double *v, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

// what the host keeps per stream between the kernels
struct SfStream {
  af_speech_features_row row = {};
  std::vector<double> frame_db, post;
  std::vector<uint8_t> energy_active, active;
  std::vector<int32_t> listed;
};

// how many 48 kHz chunks of every stream the scratch (f64 signal and mask bytes) holds at once
int sf_segment_chunks(const af_speech_features *h, int32_t B) {
  return (int)std::max<int64_t>(1, h->scratch_bytes / ((int64_t)9 * SFM_CHUNK48 * B));
}

// resample_poly of every capture and of its sample mask (h->d_active: [B][F] frame flags) and the K-weighting behind it, a
// segment of whole chunks of all streams at a time -- the recurrence is serial in time and parallel over streams only, so the
// streams stay together and the filter states are carried in h->d_state: h->d_energy, h->d_masked_energy and h->d_count,
// [B][chunks of 960] each
template <typename Span>
int sf_resample_and_weight(af_speech_features *h, const float *d_speech, int64_t n, int32_t B, int64_t stride, Span &span, hipStream_t q) {
  const sfm_geometry &geo = h->geo;
  const int F = (int)sfm_frames_at(&geo, n), C = (int)sfm_chunks48(&geo, n);
  const int64_t n48 = sfm_resampled_length(&geo, n);
  const int segment = std::min(C, sf_segment_chunks(h, B));
  const int64_t row = (int64_t)segment * SFM_CHUNK48;
  const af::SfResamplePlan plan = {geo.up, geo.down, geo.rem, geo.taps};
  AF_HIP(h->d_resampled.reserve_exact(sizeof(double) * (size_t)B * row));
  AF_HIP(h->d_resampled_mask.reserve_exact((size_t)B * row));
  AF_HIP(h->d_state.reserve_exact(sizeof(double) * 4 * (size_t)B));
  AF_HIP(h->d_energy.reserve_exact(sizeof(double) * (size_t)B * C));
  AF_HIP(h->d_masked_energy.reserve_exact(sizeof(double) * (size_t)B * C));
  AF_HIP(h->d_count.reserve_exact(sizeof(int32_t) * (size_t)B * C));
  AF_HIP(hipMemsetAsync(h->d_state, 0, sizeof(double) * 4 * (size_t)B, q));
  for (int c0 = 0; c0 < C; c0 += segment) {
    const int chunks = std::min(C - c0, segment);
    const int64_t samples = std::min<int64_t>(n48 - (int64_t)c0 * SFM_CHUNK48, (int64_t)chunks * SFM_CHUNK48);
    AF_HIP(span(5));
    AF_HIP(af::launch_sf_resample(d_speech, stride, n, B, h->d_active, F, geo.hop, plan, h->d_phase_table, n48, c0, chunks, row,
                                  h->d_resampled, h->d_resampled_mask, h->d_count, q));
    AF_HIP(h->events.mark(q));
    AF_HIP(span(1));
    AF_HIP(af::launch_sf_kweight_resampled(h->d_resampled, h->d_resampled_mask, row, samples, B, C, c0, h->d_state, h->d_energy,
                                           h->d_masked_energy, q));
    AF_HIP(h->events.mark(q));
  }
  return AF_OK;
}

int sf_analyze(af_speech_features *h, const float *d_speech, int64_t n, int32_t B, int64_t stride, const double *noise_rms_db,
               const double *vad, int64_t n_vad, const float *d_noise, int64_t m, int64_t noise_stride,
               const af_speech_features_outputs *out) {
  const sfm_geometry &geo = h->geo;
  const bool resample = geo.up != geo.down;  // C: chunks of 960 samples at 48 kHz
  const int F = (int)sfm_frames_at(&geo, n), C = (int)sfm_chunks48(&geo, n), Fn = d_noise ? (int)sfm_frames_at(&geo, m) : 0, S = h->sib_bins;
  const int BF = af::kSfBandFields;
  hipStream_t q = nullptr;
  h->events.restart();
  h->span_kind.clear();
  const auto span = [&](int8_t kind) { h->span_kind.push_back(kind); return h->events.mark(q); };
  if (int rc = sf_upload_tables(h)) return rc;

  // 1. frame powers, then the levels and masks of every stream
  std::vector<double> power((size_t)B * F), energy((size_t)B * C);
  AF_HIP(h->d_power.reserve_exact(sizeof(double) * power.size()));
  AF_HIP(h->d_energy.reserve_exact(sizeof(double) * energy.size()));
  AF_HIP(span(0));
  AF_HIP(af::launch_sf_frame_power(d_speech, stride, B, F, geo.frame, geo.hop, h->d_power, q));
  AF_HIP(h->events.mark(q));
  AF_HIP(hipMemcpy(power.data(), h->d_power, sizeof(double) * power.size(), hipMemcpyDeviceToHost));
  std::vector<SfStream> streams((size_t)B);
  for (int s = 0; s < B; ++s) {
    SfStream &st = streams[(size_t)s];
    st.row.non_finite = !all_finite(&power[(size_t)s * F], (size_t)F);
    if (st.row.non_finite) continue;
    st.frame_db.resize((size_t)F); st.post.resize((size_t)F); st.energy_active.resize((size_t)F); st.active.resize((size_t)F);
    st.listed.resize((size_t)F);
    sfm_masks_at(&geo, &power[(size_t)s * F], F, noise_rms_db[s], vad ? vad + (int64_t)s * n_vad : nullptr, n_vad, st.frame_db.data(),
                 st.energy_active.data(), st.active.data(), st.post.data(), st.listed.data(), &st.row);
    st.listed.resize((size_t)st.row.spectral_frames);
  }

  // 2. K-weighted chunk energies at 48 kHz -- behind the resampling of signal and mask at any other rate -- and the loudness
  std::vector<double> masked_energy;
  std::vector<int32_t> count;
  if (!resample) {
    AF_HIP(span(1));
    AF_HIP(af::launch_sf_kweight(d_speech, stride, n, B, C, h->d_energy, q));
    AF_HIP(h->events.mark(q));
  } else {
    std::vector<uint8_t> flags((size_t)B * F, 0);
    for (int s = 0; s < B; ++s)
      if (!streams[(size_t)s].row.non_finite) std::memcpy(&flags[(size_t)s * F], streams[(size_t)s].active.data(), (size_t)F);
    masked_energy.resize((size_t)B * C);
    count.resize((size_t)B * C);
    AF_HIP(h->d_active.reserve_exact(flags.size()));
    AF_HIP(hipMemcpy(h->d_active, flags.data(), flags.size(), hipMemcpyHostToDevice));
    if (int rc = sf_resample_and_weight(h, d_speech, n, B, stride, span, q)) return rc;
    AF_HIP(hipMemcpy(masked_energy.data(), h->d_masked_energy, sizeof(double) * masked_energy.size(), hipMemcpyDeviceToHost));
    AF_HIP(hipMemcpy(count.data(), h->d_count, sizeof(int32_t) * count.size(), hipMemcpyDeviceToHost));
  }
  AF_HIP(hipMemcpy(energy.data(), h->d_energy, sizeof(double) * energy.size(), hipMemcpyDeviceToHost));
  int64_t max_rows = 1;
  for (int s = 0; s < B; ++s) {
    SfStream &st = streams[(size_t)s];
    if (st.row.non_finite) continue;
    if (!all_finite(&energy[(size_t)s * C], (size_t)C)) {  // a non-finite sample behind the last frame
      st.row = af_speech_features_row{};
      st.row.non_finite = 1;
      continue;
    }
    if (!resample) sfm_loudness(&energy[(size_t)s * C], n, st.active.data(), F, &st.row);
    else sfm_loudness_at(&geo, &energy[(size_t)s * C], &masked_energy[(size_t)s * C], &count[(size_t)s * C], n, st.active.data(), F, &st.row);
    max_rows = std::max<int64_t>(max_rows, st.row.spectral_frames);
  }

  // 3. frame spectra, medians, the frame model and the candidate spectrum, a tile of streams at a time
  const int64_t budget_rows = std::max<int64_t>(1, ((int64_t)256 << 20) / (int64_t)(sizeof(double) * (size_t)S));
  const int tile = (int)std::min<int64_t>(af::kSfTileStreams, std::max<int64_t>(1, budget_rows / max_rows));
  std::vector<af::SfFrameItem> items;
  std::vector<af::VsMedianJob> jobs, noise_jobs;
  std::vector<af::SfPeakJob> peak_jobs;
  std::vector<int32_t> first_row, sib_arg, arg;
  std::vector<double> band, sib_mid, noise_band, band_mid, noise_mid, weights, sums, features, probabilities;
  for (int t0 = 0; t0 < B; t0 += tile) {
    const int t1 = std::min(B, t0 + tile), T = t1 - t0;
    items.clear(); jobs.clear(); noise_jobs.clear(); peak_jobs.clear(); first_row.clear();
    int32_t R = 0, Rn = 0;
    for (int s = t0; s < t1; ++s) {
      const SfStream &st = streams[(size_t)s];
      first_row.push_back(R);
      if (st.row.non_finite) continue;
      const int A = st.row.spectral_frames;
      for (int i = 0; i < A; ++i) items.push_back({1, s, st.listed[(size_t)i], R + i});
      if (A) jobs.push_back({R, A, s - t0, 0});
      R += A;
    }
    for (int s = t0; s < t1; ++s) {  // the noise frames behind the speech frames; rows of their own
      if (streams[(size_t)s].row.non_finite || !Fn) continue;
      for (int f = 0; f < Fn; ++f) items.push_back({0, s, f, (s - t0) * Fn + f});
      noise_jobs.push_back({(s - t0) * Fn, Fn, s - t0, 0});
      Rn = T * Fn;
    }
    band.assign((size_t)std::max(R, 1) * BF, 0.0);
    sib_mid.assign((size_t)std::max(R, 1) * 2, 0.0);
    sib_arg.assign((size_t)std::max(R, 1), 0);
    noise_band.assign((size_t)std::max(Rn, 1), 0.0);
    band_mid.assign((size_t)T * 2 * BF, 0.0);
    noise_mid.assign((size_t)T * 2, 0.0);
    weights.assign((size_t)std::max(R, 1), 0.0);
    features.assign((size_t)std::max(R, 1) * SFM_FEATURES, 0.0);
    probabilities.assign((size_t)std::max(R, 1), 0.0);
    sums.assign((size_t)T * S, 0.0);
    arg.assign((size_t)T, 0);
    if (!items.empty()) {
      AF_HIP(h->d_band.reserve_exact(sizeof(double) * band.size()));
      AF_HIP(h->d_sib_mid.reserve_exact(sizeof(double) * sib_mid.size()));
      AF_HIP(h->d_sib_arg.reserve_exact(sizeof(int32_t) * sib_arg.size()));
      AF_HIP(h->d_sib_rows.reserve_exact(sizeof(double) * (size_t)std::max(R, 1) * S));
      AF_HIP(h->d_noise_band.reserve_exact(sizeof(double) * noise_band.size()));
      AF_HIP(h->d_band_mid.reserve_exact(sizeof(double) * band_mid.size()));
      AF_HIP(h->d_noise_mid.reserve_exact(sizeof(double) * noise_mid.size()));
      AF_HIP(h->d_items.reserve_exact(sizeof(af::SfFrameItem) * items.size()));
      AF_HIP(h->d_jobs.reserve_exact(sizeof(af::VsMedianJob) * std::max<size_t>(1, jobs.size())));
      AF_HIP(h->d_noise_jobs.reserve_exact(sizeof(af::VsMedianJob) * std::max<size_t>(1, noise_jobs.size())));
      AF_HIP(hipMemcpy(h->d_items, items.data(), sizeof(af::SfFrameItem) * items.size(), hipMemcpyHostToDevice));
      if (!jobs.empty()) AF_HIP(hipMemcpy(h->d_jobs, jobs.data(), sizeof(af::VsMedianJob) * jobs.size(), hipMemcpyHostToDevice));
      if (!noise_jobs.empty())
        AF_HIP(hipMemcpy(h->d_noise_jobs, noise_jobs.data(), sizeof(af::VsMedianJob) * noise_jobs.size(), hipMemcpyHostToDevice));
      AF_HIP(span(2));
      AF_HIP(af::launch_sf_frames(d_speech, stride, d_noise, noise_stride, h->d_items, (int32_t)items.size(), geo.hop, h->plan, h->bands, h->d_window,
                                  h->d_twiddles, h->d_band, h->d_sib_mid, h->d_sib_arg, h->d_sib_rows, h->d_noise_band, q));
      AF_HIP(h->events.mark(q));
      AF_HIP(span(3));
      AF_HIP(af::launch_vs_median(h->d_band, h->d_jobs, (int32_t)jobs.size(), BF, h->d_band_mid, q));
      AF_HIP(af::launch_vs_median(h->d_noise_band, h->d_noise_jobs, (int32_t)noise_jobs.size(), 1, h->d_noise_mid, q));
      AF_HIP(h->events.mark(q));
      if (R) {
        AF_HIP(hipMemcpy(band.data(), h->d_band, sizeof(double) * (size_t)R * BF, hipMemcpyDeviceToHost));
        AF_HIP(hipMemcpy(sib_mid.data(), h->d_sib_mid, sizeof(double) * (size_t)R * 2, hipMemcpyDeviceToHost));
        AF_HIP(hipMemcpy(sib_arg.data(), h->d_sib_arg, sizeof(int32_t) * (size_t)R, hipMemcpyDeviceToHost));
      }
      if (Rn) AF_HIP(hipMemcpy(noise_band.data(), h->d_noise_band, sizeof(double) * (size_t)Rn, hipMemcpyDeviceToHost));
      if (!jobs.empty()) AF_HIP(hipMemcpy(band_mid.data(), h->d_band_mid, sizeof(double) * band_mid.size(), hipMemcpyDeviceToHost));
      if (!noise_jobs.empty()) AF_HIP(hipMemcpy(noise_mid.data(), h->d_noise_mid, sizeof(double) * noise_mid.size(), hipMemcpyDeviceToHost));
    }
    for (int s = t0; s < t1; ++s) {  // the frame model of every stream, then the weights of its candidate spectrum
      SfStream &st = streams[(size_t)s];
      if (st.row.non_finite) continue;
      const int A = st.row.spectral_frames, r0 = first_row[(size_t)(s - t0)];
      if (Fn && !all_finite(&noise_band[(size_t)(s - t0) * Fn], (size_t)Fn)) {
        st.row = af_speech_features_row{};
        st.row.non_finite = 1;
        continue;
      }
      sfm_evidence(h->model, A, st.listed.data(), &band[(size_t)r0 * BF], &sib_mid[(size_t)r0 * 2], &sib_arg[(size_t)r0],
                   st.row.vad_probability_used ? st.post.data() : nullptr, &band_mid[(size_t)(s - t0) * 2 * BF], Fn,
                   &noise_mid[(size_t)(s - t0) * 2], h->freqs.data() + h->bands.first[af::kSfSibBand], &features[(size_t)r0 * SFM_FEATURES],
                   &probabilities[(size_t)r0], &weights[(size_t)r0], &st.row);
      if (A) peak_jobs.push_back({r0, A, s - t0, 0});
    }
    if (!peak_jobs.empty()) {
      AF_HIP(h->d_weights.reserve_exact(sizeof(double) * weights.size()));
      AF_HIP(h->d_sums.reserve_exact(sizeof(double) * sums.size()));
      AF_HIP(h->d_arg.reserve_exact(sizeof(int32_t) * arg.size()));
      AF_HIP(h->d_peak_jobs.reserve_exact(sizeof(af::SfPeakJob) * peak_jobs.size()));
      AF_HIP(hipMemcpy(h->d_weights, weights.data(), sizeof(double) * (size_t)R, hipMemcpyHostToDevice));
      AF_HIP(hipMemcpy(h->d_peak_jobs, peak_jobs.data(), sizeof(af::SfPeakJob) * peak_jobs.size(), hipMemcpyHostToDevice));
      AF_HIP(hipMemset(h->d_sums, 0, sizeof(double) * sums.size()));
      AF_HIP(hipMemset(h->d_arg, 0, sizeof(int32_t) * arg.size()));
      AF_HIP(span(4));
      AF_HIP(af::launch_sf_weighted_peak(h->d_sib_rows, h->d_weights, h->d_peak_jobs, (int32_t)peak_jobs.size(), S, h->d_sums, h->d_arg, q));
      AF_HIP(h->events.mark(q));
      AF_HIP(hipMemcpy(sums.data(), h->d_sums, sizeof(double) * sums.size(), hipMemcpyDeviceToHost));
      AF_HIP(hipMemcpy(arg.data(), h->d_arg, sizeof(int32_t) * arg.size(), hipMemcpyDeviceToHost));
    }
    for (int s = t0; s < t1; ++s) {
      SfStream &st = streams[(size_t)s];
      const int A = st.row.non_finite ? 0 : st.row.spectral_frames, r0 = first_row[(size_t)(s - t0)];
      if (A) st.row.peak_hz = h->freqs[(size_t)(h->bands.first[af::kSfSibBand] + arg[(size_t)(s - t0)])];  // :398-402
      if (out->rows) out->rows[s] = st.row;
      if (st.row.non_finite) continue;
      const size_t o = (size_t)s * F;
      if (out->frame_db) std::memcpy(out->frame_db + o, st.frame_db.data(), sizeof(double) * (size_t)F);
      if (out->active_frame_mask) std::memcpy(out->active_frame_mask + o, st.active.data(), (size_t)F);
      if (out->frame_indices && A) std::memcpy(out->frame_indices + o, st.listed.data(), sizeof(int32_t) * (size_t)A);
      if (out->frame_probabilities && A) std::memcpy(out->frame_probabilities + o, &probabilities[(size_t)r0], sizeof(double) * (size_t)A);
      if (out->frame_feature_rows && A)
        std::memcpy(out->frame_feature_rows + o * SFM_FEATURES, &features[(size_t)r0 * SFM_FEATURES], sizeof(double) * (size_t)A * SFM_FEATURES);
      if (out->band_sums && A) std::memcpy(out->band_sums + o * BF, &band[(size_t)r0 * BF], sizeof(double) * (size_t)A * BF);
      if (out->sibilance_middles && A) std::memcpy(out->sibilance_middles + o * 2, &sib_mid[(size_t)r0 * 2], sizeof(double) * (size_t)A * 2);
      if (out->sibilance_argmax && A) std::memcpy(out->sibilance_argmax + o, &sib_arg[(size_t)r0], sizeof(int32_t) * (size_t)A);
      if (out->sibilance_rows && A)
        AF_HIP(hipMemcpy(out->sibilance_rows + o * S, h->d_sib_rows + (size_t)r0 * S, sizeof(double) * (size_t)A * S, hipMemcpyDeviceToHost));
      if (out->noise_band_sums && Fn)
        std::memcpy(out->noise_band_sums + (size_t)s * Fn, &noise_band[(size_t)(s - t0) * Fn], sizeof(double) * (size_t)Fn);
      if (out->weighted_sums && A) std::memcpy(out->weighted_sums + (size_t)s * S, &sums[(size_t)(s - t0) * S], sizeof(double) * (size_t)S);
      if (out->weighted_argmax && A) out->weighted_argmax[s] = arg[(size_t)(s - t0)];
    }
  }
  AF_HIP(hipStreamSynchronize(q));
  if (out->frame_power) std::memcpy(out->frame_power, power.data(), sizeof(double) * power.size());
  if (out->chunk_energy) std::memcpy(out->chunk_energy, energy.data(), sizeof(double) * energy.size());
  return AF_OK;
}

}  // namespace

namespace af {

int sf_create(const sfm_geometry &geo, int32_t max_streams, int64_t max_speech_samples, int64_t max_noise_samples, int32_t device,
              af_speech_features **out) {
  if (max_streams <= 0) return fail(AF_ERR_INVALID_ARGUMENT, "max_streams must be positive");
  if (max_speech_samples < geo.frame)
    return fail(AF_ERR_INVALID_ARGUMENT, "max_speech_samples must hold one analysis frame of %d samples", geo.frame);
  if (max_noise_samples < 0) return fail(AF_ERR_INVALID_ARGUMENT, "max_noise_samples must be >= 0");
  if (device < 0) return fail(AF_ERR_INVALID_ARGUMENT, "device must be >= 0");
  NrPlan plan;
  const SfResamplePlan resample = {geo.up, geo.down, geo.rem, geo.taps};
  if (geo.frame != 2 * geo.hop || geo.hop > kSfMaxHop || !nr_make_plan(geo.hop, plan) ||
      (geo.up != geo.down && sf_resample_span(resample) > kSfResampleSpan))
    return fail(AF_ERR_UNSUPPORTED, "sample rate %d Hz: its analysis frame of %d samples does not fit the frame transform", geo.rate, geo.frame);
  af_speech_features *h = new af_speech_features();
  h->device = device;
  h->max_streams = max_streams;
  h->max_speech = max_speech_samples;
  h->max_noise = max_noise_samples;
  h->geo = geo;
  h->plan = plan;  // 960 = 5 3 2^6 at 48 kHz
  h->model[0] = SFM_FRAME_INTERCEPT;
  std::copy(sfm_frame_coefficients, sfm_frame_coefficients + SFM_FEATURES, h->model + 1);
  double sumw2 = 0.0;
  nr_make_window(geo.frame, h->window, &sumw2);
  nr_make_twiddles(geo.frame, h->twiddles);
  nr_freqs((uint32_t)geo.rate, geo.frame, h->freqs);
  sf_make_bands((uint32_t)geo.rate, h->freqs, h->bands);
  h->sib_bins = h->bands.last[kSfSibBand] - h->bands.first[kSfSibBand] + 1;
  if (geo.up != geo.down) {
    h->phase_table.resize((size_t)geo.up * geo.taps);
    sfm_polyphase_table(&geo, h->phase_table.data());
  }
  *out = h;
  return AF_OK;
}

int sf_set_frame_model(af_speech_features *h, double intercept, const double *coefficients) {
  if (!h || !coefficients) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  if (!std::isfinite(intercept) || !all_finite(coefficients, SFM_FEATURES))
    return fail(AF_ERR_INVALID_ARGUMENT, "frame model parameters must be finite");
  h->model[0] = intercept;
  std::copy(coefficients, coefficients + SFM_FEATURES, h->model + 1);
  return AF_OK;
}

int sf_get_frame_model(const af_speech_features *h, double *intercept, double *coefficients) {
  if (!h || !intercept || !coefficients) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  *intercept = h->model[0];
  std::copy(h->model + 1, h->model + 1 + SFM_FEATURES, coefficients);
  return AF_OK;
}

int sf_set_scratch_bytes(af_speech_features *h, int64_t bytes) {
  if (!h) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  if (bytes < 1 || bytes > ((int64_t)1 << 40)) return fail(AF_ERR_INVALID_ARGUMENT, "scratch bytes must be 1 .. 2^40");
  h->scratch_bytes = bytes;
  return AF_OK;
}

int sf_analyze_device(af_speech_features *h, const float *d_speech, int64_t n_speech, int32_t n_streams, int64_t speech_stride,
                      const double *noise_rms_db, const double *vad_probabilities, int64_t n_vad, const float *d_noise, int64_t n_noise,
                      int64_t noise_stride, const af_speech_features_outputs *out) {
  if (int rc = sf_check(h, d_speech, n_speech, n_streams, speech_stride, noise_rms_db, vad_probabilities, n_vad, d_noise, n_noise,
                        noise_stride, out))
    return rc;
  AF_HIP(hipSetDevice(h->device));
  h->touched_device = true;
  return sf_analyze(h, d_speech, n_speech, n_streams, speech_stride, noise_rms_db, vad_probabilities, n_vad, d_noise, d_noise ? n_noise : 0,
                    noise_stride, out);
}

int sf_analyze_host(af_speech_features *h, const float *speech, int64_t n_speech, int32_t n_streams, int64_t speech_stride,
                    const double *noise_rms_db, const double *vad_probabilities, int64_t n_vad, const float *noise, int64_t n_noise,
                    int64_t noise_stride, const af_speech_features_outputs *out) {
  if (int rc = sf_check(h, speech, n_speech, n_streams, speech_stride, noise_rms_db, vad_probabilities, n_vad, noise, n_noise, noise_stride,
                        out))
    return rc;
  AF_HIP(hipSetDevice(h->device));
  h->touched_device = true;
  const size_t f4 = sizeof(float);
  const bool with_noise = noise && n_noise > 0;
  AF_HIP(h->d_speech.reserve_exact(f4 * (size_t)n_streams * n_speech));  // (every call synchronises before it returns)
  AF_HIP(hipMemcpy2D(h->d_speech, f4 * n_speech, speech, f4 * speech_stride, f4 * n_speech, n_streams, hipMemcpyHostToDevice));
  if (with_noise) {
    AF_HIP(h->d_noise.reserve_exact(f4 * (size_t)n_streams * n_noise));
    AF_HIP(hipMemcpy2D(h->d_noise, f4 * n_noise, noise, f4 * noise_stride, f4 * n_noise, n_streams, hipMemcpyHostToDevice));
  }
  return sf_analyze(h, h->d_speech, n_speech, n_streams, n_speech, noise_rms_db, vad_probabilities, n_vad,
                    with_noise ? h->d_noise.get() : nullptr, with_noise ? n_noise : 0, n_noise, out);
}

int sf_last_kernel_ms(af_speech_features *h, double *ms, int32_t capacity, int32_t spans) {
  if (!h || !ms) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  if (capacity < spans) return fail(AF_ERR_INVALID_ARGUMENT, "ms must hold %d values", spans);
  std::fill(ms, ms + spans, 0.0);
  if (h->events.marks() == 0) return AF_OK;
  AF_HIP(hipSetDevice(h->device));
  AF_HIP(h->events.wait_last());
  for (size_t i = 0; i < h->span_kind.size() && 2 * i + 1 < h->events.marks(); ++i) {
    double span = 0.0;
    AF_HIP(h->events.elapsed(2 * i, 2 * i + 1, &span));
    if (h->span_kind[i] < spans) ms[h->span_kind[i]] += span;
  }
  return AF_OK;
}

int sf_debug_resample_host(af_speech_features *h, const float *speech, int64_t n, int32_t B, int64_t stride, const uint8_t *active_frames,
                           double *signal, uint8_t *mask, int32_t *counts) {
  if (!h || !speech || !active_frames || !signal || !mask || !counts) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  if (h->geo.up == h->geo.down) return fail(AF_ERR_INVALID_ARGUMENT, "a 48000 Hz handle does not resample");
  if (B <= 0 || B > h->max_streams) return fail(AF_ERR_INVALID_ARGUMENT, "n_streams %d must be 1 .. max_streams %d", B, h->max_streams);
  if (n < h->geo.frame || n > h->max_speech || stride < n)
    return fail(AF_ERR_INVALID_ARGUMENT, "n_speech %lld must be one frame of %d .. max_speech_samples %lld within its stride", (long long)n,
                h->geo.frame, (long long)h->max_speech);
  AF_HIP(hipSetDevice(h->device));
  h->touched_device = true;
  const sfm_geometry &geo = h->geo;
  const int F = (int)sfm_frames_at(&geo, n), C = (int)sfm_chunks48(&geo, n);
  const int64_t n48 = sfm_resampled_length(&geo, n);
  const int segment = std::min(C, sf_segment_chunks(h, B));
  const int64_t row = (int64_t)segment * SFM_CHUNK48;
  const SfResamplePlan plan = {geo.up, geo.down, geo.rem, geo.taps};
  const size_t f4 = sizeof(float);
  if (int rc = sf_upload_tables(h)) return rc;
  AF_HIP(h->d_speech.reserve_exact(f4 * (size_t)B * n));
  AF_HIP(hipMemcpy2D(h->d_speech, f4 * n, speech, f4 * stride, f4 * n, B, hipMemcpyHostToDevice));
  AF_HIP(h->d_active.reserve_exact((size_t)B * F));
  AF_HIP(hipMemcpy(h->d_active, active_frames, (size_t)B * F, hipMemcpyHostToDevice));
  AF_HIP(h->d_resampled.reserve_exact(sizeof(double) * (size_t)B * row));
  AF_HIP(h->d_resampled_mask.reserve_exact((size_t)B * row));
  AF_HIP(h->d_count.reserve_exact(sizeof(int32_t) * (size_t)B * C));
  for (int c0 = 0; c0 < C; c0 += segment) {
    const int chunks = std::min(C - c0, segment);
    const int64_t at = (int64_t)c0 * SFM_CHUNK48, samples = std::min<int64_t>(n48 - at, (int64_t)chunks * SFM_CHUNK48);
    AF_HIP(launch_sf_resample(h->d_speech, n, n, B, h->d_active, F, geo.hop, plan, h->d_phase_table, n48, c0, chunks, row, h->d_resampled,
                              h->d_resampled_mask, h->d_count, nullptr));
    AF_HIP(hipMemcpy2D(signal + at, sizeof(double) * n48, h->d_resampled, sizeof(double) * row, sizeof(double) * samples, B,
                       hipMemcpyDeviceToHost));
    AF_HIP(hipMemcpy2D(mask + at, (size_t)n48, h->d_resampled_mask, (size_t)row, (size_t)samples, B, hipMemcpyDeviceToHost));
  }
  AF_HIP(hipMemcpy(counts, h->d_count, sizeof(int32_t) * (size_t)B * C, hipMemcpyDeviceToHost));
  return AF_OK;
}

}  // namespace af

extern "C" {

int af_speech_features_create(uint32_t sample_rate, int32_t max_streams, int64_t max_speech_samples, int64_t max_noise_samples,
                              int32_t device, af_speech_features **out) {
  if (!out) return fail(AF_ERR_INVALID_ARGUMENT, "out is null");
  *out = nullptr;
  if (sample_rate == 0) return fail(AF_ERR_INVALID_ARGUMENT, "sample_rate must be positive");
  if (sample_rate != SFM_RATE)
    return fail(AF_ERR_UNSUPPORTED,
                "sample rate %u Hz: these entry points K-weight at 48000 Hz only; the polyphase resampling the reference puts in "
                "front of that for any other rate is behind af_device_rate_features_create",
                sample_rate);
  sfm_geometry geo;
  (void)sfm_make_geometry(SFM_RATE, &geo);
  return af::sf_create(geo, max_streams, max_speech_samples, max_noise_samples, device, out);
}

void af_speech_features_destroy(af_speech_features *h) { delete h; }

int64_t af_speech_features_frames(int64_t n_samples) { return sfm_frames(n_samples); }

int64_t af_speech_features_chunks(int64_t n_samples) { return n_samples > 0 ? sfm_chunks(n_samples) : 0; }

int32_t af_speech_features_sibilance_bins(const af_speech_features *h) { return h ? h->sib_bins : 0; }

int af_speech_features_set_frame_model(af_speech_features *h, double intercept, const double coefficients[6]) {
  return af::sf_set_frame_model(h, intercept, coefficients);
}

int af_speech_features_get_frame_model(const af_speech_features *h, double *intercept, double coefficients[6]) {
  return af::sf_get_frame_model(h, intercept, coefficients);
}

int af_speech_features_analyze_device(af_speech_features *h, const float *d_speech, int64_t n_speech, int32_t n_streams,
                                      int64_t speech_stride, const double *noise_rms_db, const double *vad_probabilities, int64_t n_vad,
                                      const float *d_noise, int64_t n_noise, int64_t noise_stride, const af_speech_features_outputs *out) {
  return af::sf_analyze_device(h, d_speech, n_speech, n_streams, speech_stride, noise_rms_db, vad_probabilities, n_vad, d_noise, n_noise,
                               noise_stride, out);
}

int af_speech_features_analyze_host(af_speech_features *h, const float *speech, int64_t n_speech, int32_t n_streams, int64_t speech_stride,
                                    const double *noise_rms_db, const double *vad_probabilities, int64_t n_vad, const float *noise,
                                    int64_t n_noise, int64_t noise_stride, const af_speech_features_outputs *out) {
  return af::sf_analyze_host(h, speech, n_speech, n_streams, speech_stride, noise_rms_db, vad_probabilities, n_vad, noise, n_noise,
                             noise_stride, out);
}

int af_speech_features_last_kernel_ms(af_speech_features *h, double *ms, int32_t capacity) {
  return af::sf_last_kernel_ms(h, ms, capacity, af::kSfSpans);
}

}  // extern "C"
