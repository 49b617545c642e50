// af_speech_features_impl.hpp -- the object behind both ABI families of the speech-feature measurement: af_speech_features_*
// (af_api_speech_features.cpp, 48 kHz only) and af_device_rate_features_* (af_api_device_rate_features.cpp, the listed device
// rates).  One state, one analysis; the geometry says whether the loudness path resamples to 48 kHz first.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "af_api_internal.hpp"
#include "af_speech_features_host.hpp"
#include "af_speech_features_math.h"
#include "af_spectrum_host.hpp"

struct af_speech_features {
  int device = 0, max_streams = 0, sib_bins = 0;
  int64_t max_speech = 0, max_noise = 0;
  int64_t scratch_bytes = (int64_t)256 << 20;  // of the resampled segment: f64 signal and mask bytes of every stream
  bool touched_device = false;
  sfm_geometry geo = {};
  double model[1 + SFM_FEATURES];
  af::NrPlan plan = {};
  af::SfBandTable bands = {};
  std::vector<double> window, twiddles, freqs, phase_table;  // phase_table: [up][taps], empty at 48 kHz
  af::DeviceBuffer<double> d_window, d_twiddles, d_phase_table;  // uploaded at the first call
  af::DeviceBuffer<float> d_speech, d_noise;                     // staging of the host entry point
  af::DeviceBuffer<double> d_power, d_energy;
  af::DeviceBuffer<double> d_resampled, d_state, d_masked_energy;  // a segment of every capture at 48 kHz; filter states; per chunk
  af::DeviceBuffer<uint8_t> d_active, d_resampled_mask;
  af::DeviceBuffer<int32_t> d_count;
  af::DeviceBuffer<double> d_band, d_sib_mid, d_sib_rows, d_noise_band, d_band_mid, d_noise_mid, d_weights, d_sums;  // per tile
  af::DeviceBuffer<int32_t> d_sib_arg, d_arg;
  af::DeviceBuffer<af::SfFrameItem> d_items;
  af::DeviceBuffer<af::VsMedianJob> d_jobs, d_noise_jobs;
  af::DeviceBuffer<af::SfPeakJob> d_peak_jobs;
  af::EventChain events;          // pairs of marks around the kernels of the last call
  std::vector<int8_t> span_kind;  // per pair: which of the stages it times
  ~af_speech_features() {
    if (touched_device) { (void)hipSetDevice(device); (void)hipDeviceSynchronize(); }
  }
};

namespace af {

constexpr int kSfSpans = 5;            // frame powers | K-weighting | frame spectra | frame medians | weighted peak
constexpr int kSfSpansWithResample = 6;  // ... | resampling

// the argument checks of a create call behind the rate's own (no HIP call), then the handle with its host tables
int sf_create(const sfm_geometry &geo, int32_t max_streams, int64_t max_speech_samples, int64_t max_noise_samples, int32_t device,
              af_speech_features **out);
int sf_set_frame_model(af_speech_features *h, double intercept, const double *coefficients);
int sf_get_frame_model(const af_speech_features *h, double *intercept, double *coefficients);
// the bound on the resampled segment's scratch (256 MB by default): at least one chunk of every stream is always taken
int sf_set_scratch_bytes(af_speech_features *h, int64_t bytes);
int sf_analyze_device(af_speech_features *h, const float *d_speech, int64_t n_speech, int32_t n_streams, int64_t speech_stride,
                      const double *noise_rms_db, const double *vad_probabilities, int64_t n_vad, const float *d_noise, int64_t n_noise,
                      int64_t noise_stride, const af_speech_features_outputs *out);
int sf_analyze_host(af_speech_features *h, const float *speech, int64_t n_speech, int32_t n_streams, int64_t speech_stride,
                    const double *noise_rms_db, const double *vad_probabilities, int64_t n_vad, const float *noise, int64_t n_noise,
                    int64_t noise_stride, const af_speech_features_outputs *out);
int sf_last_kernel_ms(af_speech_features *h, double *ms, int32_t capacity, int32_t spans);
// the resampling stage alone on host captures and given frame flags [n_streams][frames]: signal [n_streams][n48], mask bytes
// [n_streams][n48], counts [n_streams][chunks of 960]
int sf_debug_resample_host(af_speech_features *h, const float *speech, int64_t n_speech, int32_t n_streams, int64_t speech_stride,
                           const uint8_t *active_frames, double *signal, uint8_t *mask, int32_t *counts);

}  // namespace af
