// af_api_device_rate_features.cpp -- the C ABI of the speech-feature measurement at device rates (af_device_rate_features_*):
// python/mic_eq/analysis/voice_setup.py:161-458 for a capture at 16, 22.05, 24, 32, 44.1, 48, 88.2 or 96 kHz.  Frames, masks and
// frame spectra are taken at the capture's rate; the loudness K-weights at 48 kHz behind scipy.signal.resample_poly of signal
// and sample mask (:127-140, :214-230), which sf_resample_kernel restates.  The object and its analysis are
// af_speech_features_impl.hpp's; at 48000 Hz nothing is resampled and every result carries af_speech_features_*'s bits.
#include <hip/hip_runtime.h>

#include "af_speech_features_impl.hpp"

struct af_device_rate_features {
  af_speech_features *core = nullptr;
  ~af_device_rate_features() { delete core; }
};

namespace {

af_speech_features *core_of(af_device_rate_features *h) { return h ? h->core : nullptr; }

// 0 and the geometry, or the refusal that names the rate and the rule it breaks
int geometry_of(uint32_t sample_rate, sfm_geometry *geo) {
  if (sample_rate == 0) return fail(AF_ERR_INVALID_ARGUMENT, "sample_rate must be positive");
  if (sfm_make_geometry((int64_t)sample_rate, geo) == 0) return AF_OK;
  const double frame = (double)sample_rate * 0.04;
  const char *rule = "it is not one of the listed rates";
  if (frame != (double)(int64_t)frame || (int64_t)frame % 2)
    rule = "its 40 ms analysis frame is not a whole, even number of samples";
  else if ((int64_t)frame / 2 > af::kSfMaxHop)
    rule = "its 40 ms analysis frame is above the 3840 samples the frame transform holds";
  else if (sample_rate < 16000)
    rule = "it is below 16000 Hz, where the 5000 Hz sibilance band leaves the spectrum";
  return fail(AF_ERR_UNSUPPORTED,
              "sample rate %u Hz: %s (the speech features take 16000, 22050, 24000, 32000, 44100, 48000, 88200 and 96000 Hz)", sample_rate,
              rule);
}

}  // namespace

extern "C" {

int af_device_rate_features_create(uint32_t sample_rate, int32_t max_streams, int64_t max_speech_samples, int64_t max_noise_samples,
                                   int32_t device, af_device_rate_features **out) {
  if (!out) return fail(AF_ERR_INVALID_ARGUMENT, "out is null");
  *out = nullptr;
  sfm_geometry geo;
  if (int rc = geometry_of(sample_rate, &geo)) return rc;
  af_speech_features *core = nullptr;
  if (int rc = af::sf_create(geo, max_streams, max_speech_samples, max_noise_samples, device, &core)) return rc;
  *out = new af_device_rate_features();
  (*out)->core = core;
  return AF_OK;
}

void af_device_rate_features_destroy(af_device_rate_features *h) { delete h; }

int64_t af_device_rate_features_frames(const af_device_rate_features *h, int64_t n_samples) {
  return h && n_samples > 0 ? sfm_frames_at(&h->core->geo, n_samples) : 0;
}

int64_t af_device_rate_features_chunks(const af_device_rate_features *h, int64_t n_samples) {
  return h && n_samples > 0 ? sfm_chunks48(&h->core->geo, n_samples) : 0;
}

int64_t af_device_rate_features_resampled_length(const af_device_rate_features *h, int64_t n_samples) {
  return h && n_samples > 0 ? sfm_resampled_length(&h->core->geo, n_samples) : 0;
}

int32_t af_device_rate_features_sibilance_bins(const af_device_rate_features *h) { return h ? h->core->sib_bins : 0; }

int af_device_rate_features_set_frame_model(af_device_rate_features *h, double intercept, const double coefficients[6]) {
  return af::sf_set_frame_model(core_of(h), intercept, coefficients);
}

int af_device_rate_features_get_frame_model(const af_device_rate_features *h, double *intercept, double coefficients[6]) {
  return af::sf_get_frame_model(h ? h->core : nullptr, intercept, coefficients);
}

int af_device_rate_features_set_scratch_bytes(af_device_rate_features *h, int64_t bytes) {
  return af::sf_set_scratch_bytes(core_of(h), bytes);
}

int af_device_rate_features_analyze_device(af_device_rate_features *h, const float *d_speech, int64_t n_speech, int32_t n_streams,
                                           int64_t speech_stride, const double *noise_rms_db, const double *vad_probabilities,
                                           int64_t n_vad, const float *d_noise, int64_t n_noise, int64_t noise_stride,
                                           const af_speech_features_outputs *out) {
  return af::sf_analyze_device(core_of(h), d_speech, n_speech, n_streams, speech_stride, noise_rms_db, vad_probabilities, n_vad, d_noise,
                               n_noise, noise_stride, out);
}

int af_device_rate_features_analyze_host(af_device_rate_features *h, const float *speech, int64_t n_speech, int32_t n_streams,
                                         int64_t speech_stride, const double *noise_rms_db, const double *vad_probabilities, int64_t n_vad,
                                         const float *noise, int64_t n_noise, int64_t noise_stride, const af_speech_features_outputs *out) {
  return af::sf_analyze_host(core_of(h), speech, n_speech, n_streams, speech_stride, noise_rms_db, vad_probabilities, n_vad, noise, n_noise,
                             noise_stride, out);
}

int af_device_rate_features_last_kernel_ms(af_device_rate_features *h, double *ms, int32_t capacity) {
  return af::sf_last_kernel_ms(core_of(h), ms, capacity, af::kSfSpansWithResample);
}

int af_device_rate_features_debug_resample_host(af_device_rate_features *h, const float *speech, int64_t n_speech, int32_t n_streams,
                                                int64_t speech_stride, const uint8_t *active_frames, double *signal, uint8_t *mask,
                                                int32_t *counts) {
  return af::sf_debug_resample_host(core_of(h), speech, n_speech, n_streams, speech_stride, active_frames, signal, mask, counts);
}

}  // extern "C"
