// af_api_setup_verification.cpp -- the C ABI of the second-passage measurements (af_setup_verification_*).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "af_api_internal.hpp"
#include "af_setup_verification_host.hpp"
#include "af_setup_verification_math.h"
#include "af_spectrum_host.hpp"

// ------------------------------------------------------------------------------------------
// voice_setup.py:1446-1679, what is measured there beside the spectra and the speech features.  Kernels: af_setup_verification.hip;
// rules and sum orders: af_setup_verification_math.h.
struct af_setup_verification {
  int device = 0, nperseg = 0, max_streams = 0;
  af::SvGrid grid{};
  std::vector<double> freqs;
  bool touched_device = false;
  af::DeviceBuffer<double> d_freqs;
  af::DeviceBuffer<int32_t> d_presets;
  af::DeviceBuffer<int64_t> d_lengths;  // [AF_SETUP_SIGNALS][max_streams]
  af::PinnedSlots<4> uploads;           // the presets and the lengths of a call: the caller's arrays are free when it returns
  std::vector<int64_t> lengths;         // one call's [AF_SETUP_SIGNALS][max_streams], gathered for one upload
  // staging of the host entry point
  af::DeviceBuffer<double> d_spectra, d_snr;
  af::DeviceBuffer<float> d_audio[AF_SETUP_SIGNALS];
  af::DeviceBuffer<af_setup_verification_row> d_rows;
  ~af_setup_verification() {  // the device comes to rest before the members release themselves
    if (touched_device) { (void)hipSetDevice(device); (void)hipDeviceSynchronize(); }
  }
};

namespace {

int sv_check(const af_setup_verification *v, int32_t n_streams, const double *original_db, const double *before_db, const double *after_db,
             int64_t spectrum_stride, const double *after_snr_db, int64_t snr_stride, const int32_t *preset_ids,
             const af_setup_verification_audio *audio, const af_setup_verification_row *rows) {
  if (!v) return fail(AF_ERR_INVALID_ARGUMENT, "setup verification is null");
  if (n_streams < 1 || n_streams > v->max_streams)
    return fail(AF_ERR_INVALID_ARGUMENT, "n_streams must be in 1..%d, got %d", v->max_streams, n_streams);
  if (!original_db || !before_db || !after_db) return fail(AF_ERR_INVALID_ARGUMENT, "null spectrum");
  if (spectrum_stride < v->grid.bins) return fail(AF_ERR_INVALID_ARGUMENT, "spectrum_stride must cover the %d bins", v->grid.bins);
  if (after_snr_db && snr_stride < v->grid.bins) return fail(AF_ERR_INVALID_ARGUMENT, "snr_stride must cover the %d bins", v->grid.bins);
  if (!preset_ids) return fail(AF_ERR_INVALID_ARGUMENT, "preset_ids is null");
  if (!audio) return fail(AF_ERR_INVALID_ARGUMENT, "audio is null");
  if (!rows) return fail(AF_ERR_INVALID_ARGUMENT, "rows is null");
  for (int32_t s = 0; s < n_streams; ++s)
    if (preset_ids[s] < 0 || preset_ids[s] >= AF_TARGET_PRESET_COUNT)
      return fail(AF_ERR_INVALID_ARGUMENT, "Unknown target preset: %d (stream %d)", preset_ids[s], s);
  for (int k = 0; k < AF_SETUP_SIGNALS; ++k) {
    const af_setup_verification_audio &a = audio[k];
    if (!a.samples) continue;
    if (a.length < 0 || a.stride < a.length) return fail(AF_ERR_INVALID_ARGUMENT, "signal %d: stride must cover length samples", k);
    if (a.lengths)
      for (int32_t s = 0; s < n_streams; ++s)
        if (a.lengths[s] < 0 || a.lengths[s] > a.length)
          return fail(AF_ERR_INVALID_ARGUMENT, "signal %d: the length of stream %d must be in 0..%lld", k, s, (long long)a.length);
  }
  return AF_OK;
}

// both kernels behind the grid's, the presets' and the lengths' copies, all on `stream`
int sv_enqueue(af_setup_verification *v, int32_t n_streams, const double *d_original, const double *d_before, const double *d_after,
               int64_t spectrum_stride, const double *d_snr, int64_t snr_stride, const int32_t *preset_ids,
               const af_setup_verification_audio *audio, af_setup_verification_row *d_rows, hipStream_t stream) {
  AF_HIP(hipSetDevice(v->device));
  v->touched_device = true;
  const size_t B = (size_t)v->max_streams;
  if (!v->d_freqs) {
    AF_HIP(v->d_freqs.reserve_exact(sizeof(double) * v->freqs.size()));
    AF_HIP(v->d_freqs.keep_if(hipMemcpy(v->d_freqs, v->freqs.data(), sizeof(double) * v->freqs.size(), hipMemcpyHostToDevice)));
  }
  AF_HIP(v->d_presets.reserve_exact(sizeof(int32_t) * B));
  AF_HIP(v->d_lengths.reserve_exact(sizeof(int64_t) * AF_SETUP_SIGNALS * B));
  AF_HIP(v->uploads.upload(v->d_presets, preset_ids, sizeof(int32_t) * (size_t)n_streams, stream));
  af::SvAudio a{};
  bool any_lengths = false;
  v->lengths.assign(AF_SETUP_SIGNALS * B, 0);
  for (int k = 0; k < AF_SETUP_SIGNALS; ++k) {
    a.samples[k] = audio[k].samples;
    a.stride[k] = audio[k].stride;
    a.length[k] = audio[k].length;
    if (audio[k].samples && audio[k].lengths) {
      std::memcpy(v->lengths.data() + (size_t)k * B, audio[k].lengths, sizeof(int64_t) * (size_t)n_streams);
      a.lengths[k] = v->d_lengths + (size_t)k * B;
      any_lengths = true;
    }
  }
  if (any_lengths) AF_HIP(v->uploads.upload(v->d_lengths, v->lengths.data(), sizeof(int64_t) * v->lengths.size(), stream));
  AF_HIP(af::launch_setup_verification_shape(v->grid, v->d_freqs, d_original, d_before, d_after, spectrum_stride, d_snr, snr_stride,
                                             v->d_presets, d_rows, n_streams, stream));
  AF_HIP(af::launch_setup_verification_levels(a, d_rows, n_streams, stream));
  return AF_OK;
}

}  // namespace

extern "C" {

int af_setup_verification_create(uint32_t sample_rate, int32_t nperseg, int32_t max_streams, int32_t device, af_setup_verification **out) {
  if (!out) return fail(AF_ERR_INVALID_ARGUMENT, "out is null");
  *out = nullptr;
  if (sample_rate != 48000)
    return fail(AF_ERR_UNSUPPORTED, "sample rate %u: the second-passage verification is built for 48000 Hz", sample_rate);
  if (nperseg < 2 || nperseg % 2 != 0) return fail(AF_ERR_INVALID_ARGUMENT, "nperseg must be even and at least 2, got %d", nperseg);
  if (nperseg > af::kSvMaxNperseg) return fail(AF_ERR_UNSUPPORTED, "nperseg %d: the sorts are built for at most %d", nperseg, af::kSvMaxNperseg);
  if (max_streams < 1) return fail(AF_ERR_INVALID_ARGUMENT, "max_streams must be positive");
  if (device < 0) return fail(AF_ERR_INVALID_ARGUMENT, "device must be >= 0");
  af_setup_verification *v = new af_setup_verification();
  v->device = device;
  v->nperseg = nperseg;
  v->max_streams = max_streams;
  af::vs_freqs(sample_rate, nperseg, v->freqs);
  af::SvGrid &g = v->grid;
  const double *f = v->freqs.data();
  int first = 0, largest;
  g.bins = (int32_t)v->freqs.size();
  svm_bin_range(f, g.bins, SVM_MASK_LOW, SVM_MASK_HIGH, 1, &g.first, &g.count);
  for (int b = 0; b < 4; ++b) svm_bin_range(f, g.bins, svm_snr_band_edges[b][0], svm_snr_band_edges[b][1], 0, &g.band_first[b], &g.band_count[b]);
  svm_bin_range(f + g.first, g.count, 180.0, 800.0, 1, &first, &g.body_count);
  svm_bin_range(f + g.first, g.count, 1200.0, 3500.0, 1, &first, &g.presence_count);
  svm_bin_range(f + g.first, g.count, 5500.0, 8500.0, 1, &first, &g.sibilance_count);
  svm_bin_range(f + g.first, g.count, 100.0, 8000.0, 1, &first, &g.voice_count);
  largest = g.count;
  for (int b = 0; b < 4; ++b) largest = g.band_count[b] > largest ? g.band_count[b] : largest;
  g.sort_capacity = 2;
  while (g.sort_capacity < largest) g.sort_capacity *= 2;
  if (g.sort_capacity > af::kSvMaxSorted) {  // (not reachable at 48 kHz below kSvMaxNperseg)
    delete v;
    return fail(AF_ERR_UNSUPPORTED, "nperseg %d leaves %d bins to sort, more than %d", nperseg, largest, af::kSvMaxSorted);
  }
  *out = v;
  return AF_OK;
}

void af_setup_verification_destroy(af_setup_verification *v) { delete v; }

int af_setup_verification_measure_device(af_setup_verification *v, int32_t n_streams, const double *d_original_db,
                                         const double *d_before_db, const double *d_after_db, int64_t spectrum_stride,
                                         const double *d_after_snr_db, int64_t snr_stride, const int32_t *preset_ids,
                                         const af_setup_verification_audio *audio, af_setup_verification_row *d_rows, void *hip_stream) {
  if (int rc = sv_check(v, n_streams, d_original_db, d_before_db, d_after_db, spectrum_stride, d_after_snr_db, snr_stride, preset_ids,
                        audio, d_rows))
    return rc;
  return sv_enqueue(v, n_streams, d_original_db, d_before_db, d_after_db, spectrum_stride, d_after_snr_db, snr_stride, preset_ids, audio,
                    d_rows, static_cast<hipStream_t>(hip_stream));
}

int af_setup_verification_measure_host(af_setup_verification *v, int32_t n_streams, const double *original_db, const double *before_db,
                                       const double *after_db, int64_t spectrum_stride, const double *after_snr_db, int64_t snr_stride,
                                       const int32_t *preset_ids, const af_setup_verification_audio *audio,
                                       af_setup_verification_row *rows) {
  if (int rc = sv_check(v, n_streams, original_db, before_db, after_db, spectrum_stride, after_snr_db, snr_stride, preset_ids, audio, rows))
    return rc;
  AF_HIP(hipSetDevice(v->device));
  v->touched_device = true;
  const size_t B = (size_t)n_streams, K = (size_t)v->grid.bins, d8 = sizeof(double), f4 = sizeof(float);
  // (the host entry point synchronises before it returns: nothing reads the old buffers)
  AF_HIP(v->d_spectra.reserve_exact(d8 * 3 * B * K));
  AF_HIP(v->d_rows.reserve_exact(sizeof(af_setup_verification_row) * B));
  const double *src[3] = {original_db, before_db, after_db};
  for (int k = 0; k < 3; ++k)
    AF_HIP(hipMemcpy2D(v->d_spectra + (size_t)k * B * K, d8 * K, src[k], d8 * (size_t)spectrum_stride, d8 * K, B, hipMemcpyHostToDevice));
  if (after_snr_db) {
    AF_HIP(v->d_snr.reserve_exact(d8 * B * K));
    AF_HIP(hipMemcpy2D(v->d_snr, d8 * K, after_snr_db, d8 * (size_t)snr_stride, d8 * K, B, hipMemcpyHostToDevice));
  }
  af_setup_verification_audio staged[AF_SETUP_SIGNALS];
  for (int k = 0; k < AF_SETUP_SIGNALS; ++k) {
    staged[k] = audio[k];
    if (!audio[k].samples) continue;
    const size_t n = (size_t)audio[k].length, row = n ? n : 1;  // (a present signal of no samples keeps a non-null pointer)
    AF_HIP(v->d_audio[k].reserve_exact(f4 * B * row));
    if (n) AF_HIP(hipMemcpy2D(v->d_audio[k], f4 * n, audio[k].samples, f4 * (size_t)audio[k].stride, f4 * n, B, hipMemcpyHostToDevice));
    staged[k].samples = v->d_audio[k];
    staged[k].stride = (int64_t)row;
  }
  if (int rc = sv_enqueue(v, n_streams, v->d_spectra, v->d_spectra + B * K, v->d_spectra + 2 * B * K, (int64_t)K,
                          after_snr_db ? v->d_snr.get() : nullptr, (int64_t)K, preset_ids, staged, v->d_rows, nullptr))
    return rc;
  AF_HIP(hipStreamSynchronize(nullptr));
  AF_HIP(hipMemcpy(rows, v->d_rows, sizeof(af_setup_verification_row) * B, hipMemcpyDeviceToHost));
  return AF_OK;
}

int af_setup_verification_decide(const af_setup_verification_row *row, const af_setup_verification_evidence *evidence,
                                 af_setup_verification_result *out) {
  if (!row || !evidence || !out) return fail(AF_ERR_INVALID_ARGUMENT, "null row, evidence or result");
  if (!(evidence->sample_rate > 0.0)) return fail(AF_ERR_INVALID_ARGUMENT, "sample_rate must be positive");
  if (evidence->verification_samples < 0) return fail(AF_ERR_INVALID_ARGUMENT, "verification_samples must be >= 0");
  svm_decide(row, evidence, out);
  return AF_OK;
}

const char *af_setup_verification_reason_text(int32_t reason) {
  return reason >= 0 && reason < AF_SETUP_REASON_COUNT ? svm_reason_texts[reason] : nullptr;
}

int af_setup_offline_validation(const af_setup_offline_inputs *in, af_setup_offline_result *out) {
  if (!in || !out) return fail(AF_ERR_INVALID_ARGUMENT, "null inputs or result");
  svm_offline_validation(in, out);
  return AF_OK;
}

const char *af_setup_offline_reason_text(int32_t bit_index) {
  return bit_index >= 0 && bit_index < AF_SETUP_UNCERTAIN_COUNT ? svm_uncertainty_texts[bit_index] : nullptr;
}

}  // extern "C"
