// af_api_lane_eq.cpp -- the C ABI of the per-lane EQ (af_lane_eq_*): the EQ half of the renders behind
// python/mic_eq/analysis/auto_eq_parts/headroom.py:292-354.  The kernel is af_lane_eq.hip's; every lane's section coefficients
// and crossfade counters come from the host mirror of the reference's setters (EqProto, af_host.hpp), which the engine uses too.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "af_api_internal.hpp"
#include "af_host.hpp"
#include "af_lane_eq_host.hpp"

struct af_lane_eq {
  int device = 0;
  double sample_rate = 48000.0;
  bool touched_device = false;
  // the last run
  int32_t n_lanes = 0;
  int64_t n_samples = 0, out_stride = 0;
  af::DeviceBuffer<float> d_audio, d_out;
  af::DeviceBuffer<double> d_coef;
  af::DeviceBuffer<int32_t> d_fade, d_lane_capture;
  af::TimedSpan span;

  ~af_lane_eq() {
    if (touched_device) { (void)hipSetDevice(device); (void)hipDeviceSynchronize(); }
  }
};

namespace {

int le_run(af_lane_eq *h, const float *audio, bool on_device, int64_t n, int32_t C, int64_t stride, const int32_t *lane_capture,
           int32_t n_lanes, const double *bands) {
  if (!h || !audio || !lane_capture || !bands) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  if (n <= 0) return fail(AF_ERR_INVALID_ARGUMENT, "n_samples must be positive");
  if (C <= 0) return fail(AF_ERR_INVALID_ARGUMENT, "n_captures must be positive");
  if (n_lanes <= 0) return fail(AF_ERR_INVALID_ARGUMENT, "n_lanes must be positive");
  if (stride < n) return fail(AF_ERR_INVALID_ARGUMENT, "stride must cover n_samples");
  for (int32_t l = 0; l < n_lanes; ++l) {
    if (lane_capture[l] < 0 || lane_capture[l] >= C)
      return fail(AF_ERR_INVALID_ARGUMENT, "lane %d names capture %d of %d", l, lane_capture[l], C);
    for (int v = 0; v < 3 * af::kNumBands; ++v)
      if (!std::isfinite(bands[(size_t)l * 3 * af::kNumBands + v]))
        return fail(AF_ERR_INVALID_ARGUMENT, "lane %d: band values must be finite", l);
  }
  const int64_t LP = ((int64_t)n_lanes + af::kLanes - 1) / af::kLanes * af::kLanes;

  // every lane's EQ: ParametricEQ::new and the setters in python_api.rs:408-412's order
  std::vector<double> coef((size_t)af::kLeCoefPlanes * LP);
  std::vector<int32_t> fade((size_t)af::kLeFadePlanes * LP), lanes((size_t)LP);
  for (int64_t l = 0; l < LP; ++l) {
    const int64_t src = std::min<int64_t>(l, n_lanes - 1);  // the padding repeats the last lane
    const double *b = bands + (size_t)src * 3 * af::kNumBands;
    af::EqProto eq(h->sample_rate);
    for (int i = 0; i < af::kNumBands; ++i) {
      eq.set_band_frequency(i, b[3 * i]);
      eq.set_band_gain(i, b[3 * i + 1]);
      eq.set_band_q(i, b[3 * i + 2]);
    }
    int k = 0;
    for (int i = 0; i < af::kNumBands; ++i) {
      if (eq.bands[i].processing_sections != 1)
        return fail(AF_ERR_BACKEND, "internal: band %d of a legacy EQ has %d sections", i, eq.bands[i].processing_sections);
      const af::SectionParams sp = eq.bands[i].sections[0].section();
      const double v[10] = {sp.active.b0,  sp.active.b1,  sp.active.b2,  sp.active.a1,  sp.active.a2,
                            sp.pending.b0, sp.pending.b1, sp.pending.b2, sp.pending.a1, sp.pending.a2};
      for (int j = 0; j < 10; ++j) coef[(size_t)(10 * k + j) * LP + l] = v[j];
      fade[(size_t)(2 * k) * LP + l] = sp.xf_total;
      fade[(size_t)(2 * k + 1) * LP + l] = sp.xf_remaining;
      ++k;
    }
    lanes[(size_t)l] = lane_capture[src];
  }

  AF_HIP(hipSetDevice(h->device));
  h->touched_device = true;
  AF_HIP(hipDeviceSynchronize());  // nothing of an earlier run still reads what is replaced
  h->n_lanes = 0;
  const size_t f4 = sizeof(float);
  const int64_t out_stride = (n + 63) / 64 * 64;
  const float *d_in = audio;
  int64_t in_stride = stride;
  if (!on_device) {
    AF_HIP(h->d_audio.reserve_exact(f4 * (size_t)C * n));
    AF_HIP(hipMemcpy2D(h->d_audio, f4 * n, audio, f4 * stride, f4 * n, C, hipMemcpyHostToDevice));
    d_in = h->d_audio;
    in_stride = n;
  }
  AF_HIP(h->d_out.reserve_exact(f4 * (size_t)LP * out_stride));
  AF_HIP(h->d_coef.reserve_exact(sizeof(double) * coef.size()));
  AF_HIP(h->d_fade.reserve_exact(sizeof(int32_t) * fade.size()));
  AF_HIP(h->d_lane_capture.reserve_exact(sizeof(int32_t) * lanes.size()));
  AF_HIP(hipMemcpy(h->d_coef, coef.data(), sizeof(double) * coef.size(), hipMemcpyHostToDevice));
  AF_HIP(hipMemcpy(h->d_fade, fade.data(), sizeof(int32_t) * fade.size(), hipMemcpyHostToDevice));
  AF_HIP(hipMemcpy(h->d_lane_capture, lanes.data(), sizeof(int32_t) * lanes.size(), hipMemcpyHostToDevice));

  af::LaneEqArgs a{};
  a.in = d_in;
  a.out = h->d_out;
  a.coef = h->d_coef;
  a.fade = h->d_fade;
  a.lane_capture = h->d_lane_capture;
  a.in_stride = in_stride;
  a.out_stride = out_stride;
  a.n_samples = n;
  a.n_lanes = n_lanes;
  a.lanes_padded = (int32_t)LP;
  hipStream_t q = nullptr;
  AF_HIP(h->span.begin(q));
  AF_HIP(af::launch_lane_eq(a, q));
  AF_HIP(h->span.end(q));
  h->n_samples = n;
  h->out_stride = out_stride;
  h->n_lanes = n_lanes;
  return AF_OK;
}

}  // namespace

extern "C" {

int af_lane_eq_create(double sample_rate, int32_t device, af_lane_eq **out) {
  if (!out) return fail(AF_ERR_INVALID_ARGUMENT, "out is null");
  *out = nullptr;
  if (!std::isfinite(sample_rate) || sample_rate <= 0.0) return fail(AF_ERR_INVALID_ARGUMENT, "sample_rate must be positive and finite");
  if (device < 0) return fail(AF_ERR_INVALID_ARGUMENT, "device must be >= 0");
  af_lane_eq *h = new af_lane_eq();
  h->sample_rate = sample_rate;
  h->device = device;
  *out = h;
  return AF_OK;
}

void af_lane_eq_destroy(af_lane_eq *h) { delete h; }

int af_lane_eq_run_host(af_lane_eq *h, const float *audio, int64_t n_samples, int32_t n_captures, int64_t stride,
                        const int32_t *lane_capture, int32_t n_lanes, const double *bands) {
  return le_run(h, audio, false, n_samples, n_captures, stride, lane_capture, n_lanes, bands);
}

int af_lane_eq_run_device(af_lane_eq *h, const float *d_audio, int64_t n_samples, int32_t n_captures, int64_t stride,
                          const int32_t *lane_capture, int32_t n_lanes, const double *bands) {
  return le_run(h, d_audio, true, n_samples, n_captures, stride, lane_capture, n_lanes, bands);
}

int af_lane_eq_output(af_lane_eq *h, float **d_out, int64_t *stride) {
  if (!h || !d_out || !stride) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  if (h->n_lanes == 0) return fail(AF_ERR_STATE, "no run has been made");
  *d_out = h->d_out;
  *stride = h->out_stride;
  return AF_OK;
}

int af_lane_eq_read_output(af_lane_eq *h, float *out, int64_t stride) {
  if (!h || !out) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  if (h->n_lanes == 0) return fail(AF_ERR_STATE, "no run has been made");
  if (stride < h->n_samples) return fail(AF_ERR_INVALID_ARGUMENT, "stride must cover n_samples");
  AF_HIP(hipSetDevice(h->device));
  const size_t f4 = sizeof(float);
  AF_HIP(hipMemcpy2D(out, f4 * stride, h->d_out, f4 * h->out_stride, f4 * h->n_samples, h->n_lanes, hipMemcpyDeviceToHost));
  return AF_OK;
}

int af_lane_eq_last_kernel_ms(af_lane_eq *h, double *ms) {
  if (!h || !ms) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  *ms = 0.0;
  if (!h->span.used()) return AF_OK;
  AF_HIP(hipSetDevice(h->device));
  AF_HIP(h->span.elapsed_ms(ms));
  return AF_OK;
}

}  // extern "C"
