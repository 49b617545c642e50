// af_api_resampler.cpp -- the C ABI of the product resampler (af_resampler_*).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "af_api_internal.hpp"
#include "af_resampler_host.hpp"
#include "af_switches.hpp"

namespace af {
hipError_t launch_resample(const double *in, double *out, const ResamplePos *pos, const double *table, int64_t n_in,
                           int64_t n_out, int64_t in_stride, int64_t out_stride, int32_t n_streams, int32_t sinc_len,
                           double ratio, int variant, hipStream_t stream);
int resample_segment_outputs(double ratio, int sinc_len);
}  // namespace af

// ------------------------------------------------------------------------------------------
// Product resampler (rust-core/src/audio/processor/resampling.rs:140-261)
struct af_resampler {
  af::ResamplePlan plan;
  int device = 0;
  std::vector<af::ResamplePos> pos;
  int64_t planned_n_in = -1, planned_n_out = 0, planned_blocks = 0, uploaded_n_in = -1;
  bool touched_device = false;  // a call allocated (or may have): the destructor has a device to wait for
  af::DeviceBuffer<double> d_table;
  af::DeviceBuffer<af::ResamplePos> d_pos;
  af::DeviceBuffer<double> d_in, d_out;  // staging of the host entry point
  af::TimedSpan span;
  int variant = 0;  // 0: matrix-core kernel (64 streams per workgroup) when the shape allows; AF_RESAMPLER_VARIANT=valu -> 1: vector kernel, =mfma32 -> 2: matrix-core kernel with 32 streams per workgroup
  ~af_resampler() {  // the device comes to rest before the members release themselves
    if (touched_device) { (void)hipSetDevice(device); (void)hipDeviceSynchronize(); }
  }
};

namespace {
// host only: replay the reference's chunk loop for n_in frames
int resampler_plan(af_resampler *r, int64_t n_in) {
  if (r->planned_n_in == n_in) return AF_OK;
  r->planned_n_out = r->plan.positions(n_in, r->pos, &r->planned_blocks);
  r->planned_n_in = n_in;
  r->uploaded_n_in = -1;
  return AF_OK;
}
// device side of the plan: coefficient table (once) and the position records of the current plan
int resampler_upload(af_resampler *r) {
  AF_HIP(hipSetDevice(r->device));
  if (!r->d_table) {
    AF_HIP(r->d_table.reserve_exact(sizeof(double) * r->plan.table.size()));
    AF_HIP(r->d_table.keep_if(hipMemcpy(r->d_table, r->plan.table.data(), sizeof(double) * r->plan.table.size(), hipMemcpyHostToDevice)));
  }
  if (r->uploaded_n_in == r->planned_n_in) return AF_OK;
  AF_HIP(r->d_pos.reserve_exact(sizeof(af::ResamplePos) * r->planned_n_out));  // (freeing the old records waits for whatever still reads them)
  if (r->planned_n_out > 0)
    AF_HIP(hipMemcpy(r->d_pos, r->pos.data(), sizeof(af::ResamplePos) * r->planned_n_out, hipMemcpyHostToDevice));
  r->uploaded_n_in = r->planned_n_in;
  return AF_OK;
}
}  // namespace

// the argument checks of simulate_product_resampler, resampling.rs:187-214, and what the kernels' LDS tiles hold; host only.
// Not part of the ABI: hidden, declared in af_api_internal.hpp for af_api_stream_resampler.cpp, which creates with the same checks.
int af_resampler_check_arguments(uint32_t input_rate, uint32_t output_rate, int64_t chunk_size, int32_t sinc_len, int32_t window,
                                 int32_t device) {
  if (input_rate == 0 || output_rate == 0) return fail(AF_ERR_INVALID_ARGUMENT, "sample rates must be positive");
  if (chunk_size < 1 || chunk_size > 1024) return fail(AF_ERR_INVALID_ARGUMENT, "chunk_size must be between 1 and 1024");
  if (sinc_len < 32 || sinc_len > 2048 || (sinc_len & (sinc_len - 1)) != 0)
    return fail(AF_ERR_INVALID_ARGUMENT, "sinc_len must be a power of two between 32 and 2048");
  if (window < 0 || window > af::kWinHann2) return fail(AF_ERR_INVALID_ARGUMENT, "unsupported resampler window %d", window);
  if (device < 0) return fail(AF_ERR_INVALID_ARGUMENT, "device must be >= 0");
  const double ratio = (double)output_rate / (double)input_rate;
  if (chunk_size <= (int64_t)sinc_len + 1 + (int64_t)std::ceil(1.0 / ratio))
    return fail(AF_ERR_UNSUPPORTED, "chunk_size %lld is too short for sinc_len %d: the reference's chunk loop would produce no frames",
                (long long)chunk_size, sinc_len);
  if (af::resample_segment_outputs(ratio, sinc_len) == 0)
    return fail(AF_ERR_UNSUPPORTED, "sinc_len %d at ratio %.4f needs a longer input span than the LDS tile holds", sinc_len, ratio);
  return AF_OK;
}

extern "C" {

int af_resampler_calculate_cutoff(int32_t sinc_len, int32_t window, float *out) {
  if (!out) return fail(AF_ERR_INVALID_ARGUMENT, "out is null");
  if (window < 0 || window > af::kWinHann2) return fail(AF_ERR_INVALID_ARGUMENT, "unsupported resampler window %d", window);
  *out = af::resample_calculate_cutoff(sinc_len, window);
  return AF_OK;
}

int af_resampler_create(uint32_t input_rate, uint32_t output_rate, int64_t chunk_size, int32_t sinc_len, int32_t window,
                        int32_t device, af_resampler **out) {
  if (!out) return fail(AF_ERR_INVALID_ARGUMENT, "out is null");
  *out = nullptr;
  if (int rc = af_resampler_check_arguments(input_rate, output_rate, chunk_size, sinc_len, window, device)) return rc;
  af_resampler *r = new af_resampler();
  r->device = device;
  r->plan.build(input_rate, output_rate, chunk_size, sinc_len, window);
  af::resampler_variant_override(r->variant);
  *out = r;
  return AF_OK;
}

void af_resampler_destroy(af_resampler *r) { delete r; }

int af_resampler_output_delay(const af_resampler *r) { return r ? r->plan.output_delay() : 0; }
int64_t af_resampler_expected_frames(const af_resampler *r, int64_t n_in) { return r ? r->plan.expected_frames(n_in) : 0; }
int af_resampler_sinc_len(const af_resampler *r) { return r ? r->plan.sinc_len : 0; }

int af_resampler_copy_sinc_table(const af_resampler *r, double *out) {
  if (!r || !out) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  const int stride = r->plan.row_stride();
  for (int row = 0; row < af::kResampleOversampling; ++row)
    std::memcpy(out + (size_t)row * r->plan.sinc_len, r->plan.table.data() + (size_t)row * stride + af::kResampleTablePad,
                sizeof(double) * r->plan.sinc_len);
  return AF_OK;
}

int af_resampler_plan(af_resampler *r, int64_t n_in, int64_t *n_out, int64_t *blocks) {
  if (!r) return fail(AF_ERR_INVALID_ARGUMENT, "resampler is null");
  if (n_in < 0) return fail(AF_ERR_INVALID_ARGUMENT, "n_in must be >= 0");
  if (int rc = resampler_plan(r, n_in)) return rc;
  if (n_out) *n_out = r->planned_n_out;
  if (blocks) *blocks = r->planned_blocks;
  return AF_OK;
}

int af_resampler_process_device(af_resampler *r, const double *d_in, double *d_out, int64_t n_in, int32_t n_streams,
                                int64_t in_stride, int64_t out_stride, void *stream) {
  if (!r) return fail(AF_ERR_INVALID_ARGUMENT, "resampler is null");
  if (n_streams <= 0) return fail(AF_ERR_INVALID_ARGUMENT, "n_streams must be positive");
  if (n_in < 0 || in_stride < n_in) return fail(AF_ERR_INVALID_ARGUMENT, "in_stride must cover n_in frames");
  if (int rc = resampler_plan(r, n_in)) return rc;
  if (out_stride < r->planned_n_out) return fail(AF_ERR_INVALID_ARGUMENT, "out_stride must cover the %lld planned output frames", (long long)r->planned_n_out);
  if ((!d_in && n_in > 0) || !d_out) return fail(AF_ERR_INVALID_ARGUMENT, "null device buffer");
  r->touched_device = true;
  if (int rc = resampler_upload(r)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  AF_HIP(r->span.begin(s));
  AF_HIP(af::launch_resample(d_in, d_out, r->d_pos, r->d_table, n_in, r->planned_n_out, in_stride, out_stride, n_streams,
                             r->plan.sinc_len, r->plan.ratio, r->variant, s));
  AF_HIP(r->span.end(s));
  return AF_OK;
}

int af_resampler_process_host(af_resampler *r, const double *in, double *out, int64_t n_in, int32_t n_streams,
                              int64_t in_stride, int64_t out_stride) {
  if (!r) return fail(AF_ERR_INVALID_ARGUMENT, "resampler is null");
  if (n_streams <= 0) return fail(AF_ERR_INVALID_ARGUMENT, "n_streams must be positive");
  if ((!in && n_in > 0) || !out) return fail(AF_ERR_INVALID_ARGUMENT, "null buffer");
  if (n_in < 0 || in_stride < n_in) return fail(AF_ERR_INVALID_ARGUMENT, "in_stride must cover n_in frames");
  if (!af::check_finite(in, n_streams, n_in, in_stride)) return fail(AF_ERR_NON_FINITE, "samples must be finite");
  if (int rc = resampler_plan(r, n_in)) return rc;
  const int64_t n_out = r->planned_n_out;
  if (out_stride < n_out) return fail(AF_ERR_INVALID_ARGUMENT, "out_stride must cover the %lld planned output frames", (long long)n_out);
  const int64_t need_in = std::max<int64_t>(1, (int64_t)n_streams * n_in), need_out = std::max<int64_t>(1, (int64_t)n_streams * n_out);
  r->touched_device = true;
  AF_HIP(r->d_in.reserve_exact(sizeof(double) * need_in));  // (this call synchronises before it returns: nothing reads the old buffers)
  AF_HIP(r->d_out.reserve_exact(sizeof(double) * need_out));
  if (n_in > 0)
    AF_HIP(hipMemcpy2D(r->d_in, sizeof(double) * n_in, in, sizeof(double) * in_stride, sizeof(double) * n_in, n_streams, hipMemcpyHostToDevice));
  if (int rc = af_resampler_process_device(r, r->d_in, r->d_out, n_in, n_streams, n_in > 0 ? n_in : 1, n_out, nullptr)) return rc;
  AF_HIP(hipStreamSynchronize(nullptr));
  if (n_out > 0)
    AF_HIP(hipMemcpy2D(out, sizeof(double) * out_stride, r->d_out, sizeof(double) * n_out, sizeof(double) * n_out, n_streams, hipMemcpyDeviceToHost));
  return AF_OK;
}

// host only: the kernel af_resampler_process_* launches for this plan (af::resample_pick_form, the launcher's own choice)
int af_resampler_launch_form(const af_resampler *r, int32_t *form, int32_t *segment_outputs, int32_t *streams_per_workgroup) {
  if (!r) return fail(AF_ERR_INVALID_ARGUMENT, "resampler is null");
  const af::ResampleForm f = af::resample_pick_form(r->plan.ratio, r->plan.sinc_len, r->variant);
  if (form) *form = f.form;
  if (segment_outputs) *segment_outputs = f.segment_outputs;
  if (streams_per_workgroup) *streams_per_workgroup = f.streams_per_workgroup;
  return AF_OK;
}

int af_resampler_last_kernel_ms(af_resampler *r, double *ms) {
  if (!r || !ms) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  AF_HIP(r->span.elapsed_ms(ms));
  return AF_OK;
}

}  // extern "C"
