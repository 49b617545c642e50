// af_api_stream_resampler.cpp -- the C ABI of the streaming product resampler (af_stream_resampler_*).
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
hipError_t launch_resample_stream(const float *plane, const float *in, float *out, const ResamplePos *pos, const double *table,
                                  int64_t split, int64_t n_in, int64_t n_out, int64_t in_stride, int64_t out_stride,
                                  int32_t plane_stride, int32_t n_streams, int32_t sinc_len, double ratio, int variant,
                                  hipStream_t stream);
hipError_t launch_resample_stream_advance(const float *plane, float *next, const float *in, int64_t split, int64_t n_in,
                                          int64_t shift, int64_t in_stride, int32_t count, int32_t plane_stride, int32_t n_streams,
                                          hipStream_t stream);
}  // namespace af

// ------------------------------------------------------------------------------------------
// The product resampler as a stream (dsp_loop.rs:274-317, 843-895, 963-1011): state carried across calls, f32 in and out.
// Kernels and the layout of the carried plane: af_resampler_stream.hip.
struct af_stream_resampler {
  af::ResamplePlan plan;
  int device = 0, n_streams = 0;
  int variant = 0;             // as af_resampler::variant
  int32_t plane_stride = 0;    // 2 * sinc_len + chunk - 1 frames per stream
  // host state: all streams advance in lock step
  double last_index = 0.0;     // SincFixedIn::last_index, advanced by the crate's repeated addition
  int64_t pending = 0;         // frames queued behind the history that do not fill a chunk yet
  int64_t chunks = 0, frames_in = 0, frames_out = 0;
  bool fresh = true;           // the history has to be zeroed in front of the next launch (create, reset)
  // device state
  bool touched_device = false;  // a push allocated (or may have): the destructor has a device to wait for
  af::DeviceBuffer<double> d_table;
  af::DeviceBuffer<float> d_plane[2];  // ping-pong pair, [n_streams][plane_stride]
  int cur = 0;
  // per-call scratch: the position records of the chunks the call completes
  std::vector<af::ResamplePos> pos;
  af::RetireList retired;      // outgrown d_pos buffers that queued launches may still read
  af::DeviceBuffer<af::ResamplePos> d_pos;
  af::PinnedSlots<8> stager;   // the records travel through pinned slots: the host never waits for a stream
  af::DeviceBuffer<float> d_in, d_out;  // staging of the host entry point
  af::TimedSpan span;
  ~af_stream_resampler() {  // the device comes to rest before the members release themselves
    if (touched_device) { (void)hipSetDevice(device); (void)hipDeviceSynchronize(); }
  }
};

namespace {

struct StreamReplay { int64_t chunks, n_out, rem; double last_index; };
// What a push of n_in frames does, replayed on the host: changes nothing.  With `pos`, the position records of the frames
// it produces, on the call's virtual axis (chunk j's buffer starts at axis frame j * chunk, its input 2 * sinc_len later).
StreamReplay stream_replay(const af_stream_resampler *r, int64_t n_in, std::vector<af::ResamplePos> *pos) {
  const int64_t total = r->pending + n_in, chunk = r->plan.chunk;
  StreamReplay p{total / chunk, 0, total % chunk, r->last_index};
  if (pos) pos->clear();
  for (int64_t j = 0; j < p.chunks; ++j)
    p.n_out += r->plan.chunk_positions(p.last_index, j * chunk + 2 * (int64_t)r->plan.sinc_len, pos);
  return p;
}

// the call's position records -> d_pos (per-call scratch) behind everything queued on `stream`
int stream_upload_positions(af_stream_resampler *r, hipStream_t stream) {
  const size_t need = sizeof(af::ResamplePos) * r->pos.size();
  AF_HIP(r->d_pos.reserve_retiring(need, r->retired, stream));
  AF_HIP(r->stager.upload(r->d_pos, r->pos.data(), need, stream));
  return AF_OK;
}

// The device half of a push whose replay `p` (with r->pos filled) has been accepted: enqueues on `stream`, commits the host state.
int stream_push_enqueue(af_stream_resampler *r, const StreamReplay &p, const float *d_in, int64_t n_in, int64_t in_stride,
                        float *d_out, int64_t out_stride, hipStream_t stream) {
  AF_HIP(hipSetDevice(r->device));
  r->touched_device = true;
  r->retired.collect(false);
  const size_t plane_bytes = sizeof(float) * (size_t)r->plane_stride * r->n_streams;
  if (!r->d_table) {
    AF_HIP(r->d_table.reserve_exact(sizeof(double) * r->plan.table.size()));
    AF_HIP(r->d_table.keep_if(hipMemcpyAsync(r->d_table, r->plan.table.data(), sizeof(double) * r->plan.table.size(), hipMemcpyHostToDevice, stream)));
  }
  if (!r->d_plane[0] || !r->d_plane[1]) {
    AF_HIP(r->d_plane[0].reserve_exact(plane_bytes));
    AF_HIP(r->d_plane[1].reserve_exact(plane_bytes));
    r->fresh = true;
  }
  if (r->fresh) {  // SincFixedIn::new / reset: a history of zeros
    AF_HIP(hipMemsetAsync(r->d_plane[r->cur], 0, plane_bytes, stream));
    r->fresh = false;
  }
  const int64_t split = 2 * (int64_t)r->plan.sinc_len + r->pending;
  if (p.n_out > 0)
    if (int rc = stream_upload_positions(r, stream)) return rc;
  AF_HIP(r->span.begin(stream));
  if (p.n_out > 0)
    AF_HIP(af::launch_resample_stream(r->d_plane[r->cur], d_in, d_out, r->d_pos, r->d_table, split, n_in, p.n_out, in_stride,
                                      out_stride, r->plane_stride, r->n_streams, r->plan.sinc_len, r->plan.ratio, r->variant, stream));
  if (n_in > 0) {  // the plane of the next call: the last 2 * sinc_len frames consumed + the remainder, into the other plane
    AF_HIP(af::launch_resample_stream_advance(r->d_plane[r->cur], r->d_plane[r->cur ^ 1], d_in, split, n_in, p.chunks * r->plan.chunk,
                                              in_stride, (int32_t)(2 * r->plan.sinc_len + p.rem), r->plane_stride, r->n_streams, stream));
    r->cur ^= 1;
  }
  AF_HIP(r->span.end(stream));
  r->last_index = p.last_index;
  r->pending = p.rem;
  r->chunks += p.chunks;
  r->frames_in += n_in;
  r->frames_out += p.n_out;
  return AF_OK;
}

// everything that can refuse a push, before anything is touched; fills r->pos
int stream_push_check(af_stream_resampler *r, const float *in, int64_t n_in, int64_t in_stride, const float *out, int64_t out_capacity,
                      int64_t out_stride, StreamReplay *p) {
  if (!r) return fail(AF_ERR_INVALID_ARGUMENT, "resampler is null");
  if (n_in < 0 || in_stride < n_in) return fail(AF_ERR_INVALID_ARGUMENT, "in_stride must cover n_in frames");
  if (!in && n_in > 0) return fail(AF_ERR_INVALID_ARGUMENT, "null buffer");
  *p = stream_replay(r, n_in, &r->pos);
  if (out_capacity < p->n_out || out_stride < p->n_out)
    return fail(AF_ERR_INVALID_ARGUMENT, "this push produces %lld frames per stream: out_capacity %lld / out_stride %lld is too small",
                (long long)p->n_out, (long long)out_capacity, (long long)out_stride);
  if (!out && p->n_out > 0) return fail(AF_ERR_INVALID_ARGUMENT, "null buffer");
  return AF_OK;
}

}  // namespace

extern "C" {

int af_stream_resampler_create(uint32_t input_rate, uint32_t output_rate, int64_t chunk_size, int32_t sinc_len, int32_t window,
                               int32_t n_streams, int32_t device, af_stream_resampler **out) {
  if (!out) return fail(AF_ERR_INVALID_ARGUMENT, "out is null");
  *out = nullptr;
  if (int rc = af_resampler_check_arguments(input_rate, output_rate, chunk_size, sinc_len, window, device)) return rc;
  if (n_streams <= 0) return fail(AF_ERR_INVALID_ARGUMENT, "n_streams must be positive");
  af_stream_resampler *r = new af_stream_resampler();
  r->device = device;
  r->n_streams = n_streams;
  r->plan.build(input_rate, output_rate, chunk_size, sinc_len, window);
  r->plane_stride = (int32_t)(2 * r->plan.sinc_len + chunk_size - 1);
  r->last_index = r->plan.initial_index();
  af::resampler_variant_override(r->variant);
  *out = r;
  return AF_OK;
}

void af_stream_resampler_destroy(af_stream_resampler *r) { delete r; }

int af_stream_resampler_reset(af_stream_resampler *r) {
  if (!r) return fail(AF_ERR_INVALID_ARGUMENT, "resampler is null");
  r->last_index = r->plan.initial_index();
  r->pending = r->chunks = r->frames_in = r->frames_out = 0;
  r->fresh = true;  // the plane is zeroed in stream order in front of the next push
  return AF_OK;
}

int af_stream_resampler_clear_pending(af_stream_resampler *r) {  // dsp_loop.rs:941-944: resample_input.clear()
  if (!r) return fail(AF_ERR_INVALID_ARGUMENT, "resampler is null");
  r->pending = 0;
  return AF_OK;
}

int64_t af_stream_resampler_output_frames(const af_stream_resampler *r, int64_t n_in) {
  if (!r || n_in < 0) return 0;
  return stream_replay(r, n_in, nullptr).n_out;
}
int64_t af_stream_resampler_pending_input(const af_stream_resampler *r) { return r ? r->pending : 0; }
int af_stream_resampler_output_delay(const af_stream_resampler *r) { return r ? r->plan.output_delay() : 0; }
int64_t af_stream_resampler_frames_in(const af_stream_resampler *r) { return r ? r->frames_in : 0; }
int64_t af_stream_resampler_frames_out(const af_stream_resampler *r) { return r ? r->frames_out : 0; }

int af_stream_resampler_push_device(af_stream_resampler *r, const float *d_in, int64_t n_in, int64_t in_stride, float *d_out,
                                    int64_t out_capacity, int64_t out_stride, int64_t *n_out, void *hip_stream) {
  if (n_out) *n_out = 0;
  StreamReplay p{};
  if (int rc = stream_push_check(r, d_in, n_in, in_stride, d_out, out_capacity, out_stride, &p)) return rc;
  if (int rc = stream_push_enqueue(r, p, d_in, n_in, in_stride, d_out, out_stride, static_cast<hipStream_t>(hip_stream))) return rc;
  if (n_out) *n_out = p.n_out;
  return AF_OK;
}

int af_stream_resampler_push_host(af_stream_resampler *r, const float *in, int64_t n_in, int64_t in_stride, float *out,
                                  int64_t out_capacity, int64_t out_stride, int64_t *n_out) {
  if (n_out) *n_out = 0;
  StreamReplay p{};
  if (int rc = stream_push_check(r, in, n_in, in_stride, out, out_capacity, out_stride, &p)) return rc;
  if (!af::check_finite(in, r->n_streams, n_in, in_stride)) return fail(AF_ERR_NON_FINITE, "samples must be finite");
  AF_HIP(hipSetDevice(r->device));
  const int64_t B = r->n_streams, need_in = std::max<int64_t>(1, B * n_in), need_out = std::max<int64_t>(1, B * p.n_out);
  r->touched_device = true;
  AF_HIP(r->d_in.reserve_exact(sizeof(float) * need_in));  // (the host entry point synchronises before it returns: nothing reads the old buffers)
  AF_HIP(r->d_out.reserve_exact(sizeof(float) * need_out));
  const size_t f4 = sizeof(float);
  if (n_in > 0) AF_HIP(hipMemcpy2D(r->d_in, f4 * n_in, in, f4 * in_stride, f4 * n_in, B, hipMemcpyHostToDevice));
  if (int rc = stream_push_enqueue(r, p, r->d_in, n_in, std::max<int64_t>(n_in, 1), r->d_out, std::max<int64_t>(p.n_out, 1), nullptr)) return rc;
  AF_HIP(hipStreamSynchronize(nullptr));
  if (p.n_out > 0) AF_HIP(hipMemcpy2D(out, f4 * out_stride, r->d_out, f4 * p.n_out, f4 * p.n_out, B, hipMemcpyDeviceToHost));
  if (n_out) *n_out = p.n_out;
  return AF_OK;
}

int af_stream_resampler_launch_form(const af_stream_resampler *r, int32_t *form, int32_t *segment_outputs,
                                    int32_t *streams_per_workgroup) {  // as af_resampler_launch_form
  if (!r) return fail(AF_ERR_INVALID_ARGUMENT, "resampler is null");
  const af::ResampleForm f = af::resample_pick_form(r->plan.ratio, r->plan.sinc_len, r->variant);
  if (form) *form = f.form;
  if (segment_outputs) *segment_outputs = f.segment_outputs;
  if (streams_per_workgroup) *streams_per_workgroup = f.streams_per_workgroup;
  return AF_OK;
}

int af_stream_resampler_last_kernel_ms(af_stream_resampler *r, double *ms) {
  if (!r || !ms) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  AF_HIP(r->span.elapsed_ms(ms));
  return AF_OK;
}

}  // extern "C"
