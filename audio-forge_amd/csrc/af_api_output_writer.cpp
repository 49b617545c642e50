// af_api_output_writer.cpp -- the C ABI of the output writer (af_output_writer_*).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "af_api_internal.hpp"
#include "af_host.hpp"
#include "af_output_writer_host.hpp"

// ------------------------------------------------------------------------------------------
// The output writer (output_writer.rs:62-343): drift retime, discontinuity fade, safety, queue accounting.  Kernels, passes
// and the state plane: af_output_writer.hip / af_output_writer_host.hpp.
struct af_output_writer {
  int device = 0, n_streams = 0;
  af_output_writer_config cfg{};
  bool limiter_enabled = true;   // live, output_writer.rs:208, 214
  float ceiling_linear = 1.0f;   // live, :209
  float release_coeff = 0.0f;    // TruePeakLimiter::default_settings(rate): 80 ms, true_peak.rs:285-287, 308-313
  bool fresh = true;             // the plane is (re)initialised in stream order in front of the next push
  bool touched_device = false;   // a push allocated (or may have): the destructor has a device to wait for
  af::DeviceBuffer<uint32_t> d_plane;
  af::DeviceBuffer<float> d_x, d_tg;      // scratch rows of the passes
  int64_t scratch_frames = 0;             // frames per stream they hold
  af::DeviceBuffer<float> d_in, d_out;    // staging of the host entry point
  af::DeviceBuffer<int64_t> d_fill, d_written;
  std::vector<float> host_rows;           // ... and its copy-back rows, kept between calls
  af::EventChain ev;  // six marks a push: before the plan pass, then behind each of the five passes
  bool timed() const { return ev.marks() == 6; }
  ~af_output_writer() {  // the device comes to rest before the members release themselves
    if (touched_device) { (void)hipSetDevice(device); (void)hipDeviceSynchronize(); }
  }
};

namespace {

int64_t ow_duration_samples(int64_t rate, int64_t ms) {  // resampling.rs:1-3
  return std::max<int64_t>((rate * ms + 500) / 1000, 1);
}

int64_t ow_max_output_frames(const af_output_writer *w, int64_t n_in) {
  // resampling.rs:92-94 at the smallest ratio; the clean path and a pass-through yield n_in
  const int64_t desired = (int64_t)std::fmax(std::round((float)n_in / af::kOwMinRatio), 1.0f);
  const int64_t retimed = std::min<int64_t>({desired, std::max<int64_t>(w->cfg.queue_capacity, 1), (int64_t)af::kOwScratch});
  return std::max(n_in, retimed);
}

int ow_push_check(af_output_writer *w, const float *in, int64_t n_in, int64_t in_stride, const int64_t *fill, const float *out,
                  int64_t out_capacity, int64_t out_stride, const int64_t *written) {
  if (!w) return fail(AF_ERR_INVALID_ARGUMENT, "output writer is null");
  if (n_in < 0) return fail(AF_ERR_INVALID_ARGUMENT, "n_in must be >= 0");
  if (n_in > af::kOwMaxBlock)
    return fail(AF_ERR_INVALID_ARGUMENT, "n_in %lld: a push takes at most %d frames", (long long)n_in, af::kOwMaxBlock);
  if (!written) return fail(AF_ERR_INVALID_ARGUMENT, "written is null");
  if (n_in == 0) return AF_OK;
  if (!in || !out || !fill) return fail(AF_ERR_INVALID_ARGUMENT, "null buffer");
  if (in_stride < n_in) return fail(AF_ERR_INVALID_ARGUMENT, "in_stride must cover n_in frames");
  const int64_t need = ow_max_output_frames(w, n_in);
  if (out_capacity < need || out_stride < need)
    return fail(AF_ERR_INVALID_ARGUMENT, "out_capacity and out_stride must cover the %lld frames a push of %lld can yield",
                (long long)need, (long long)n_in);
  return AF_OK;
}

// one write_chunk per stream, all enqueued on `stream`
int ow_enqueue(af_output_writer *w, const float *d_in, int64_t n_in, int64_t in_stride, const int64_t *d_fill, int clean_path,
               float *d_out, int64_t out_stride, int64_t *d_written, hipStream_t stream) {
  AF_HIP(hipSetDevice(w->device));
  const int B = w->n_streams;
  w->touched_device = true;
  if (!w->d_plane) {
    AF_HIP(w->d_plane.reserve_exact(sizeof(uint32_t) * af::kOwCount * (size_t)B));
    w->fresh = true;
  }
  const int64_t max_out = ow_max_output_frames(w, n_in);
  if (!w->d_x || !w->d_tg) {  // once, for the longest block a push may bring: no later push allocates or waits
    const int64_t longest = ow_max_output_frames(w, af::kOwMaxBlock);
    AF_HIP(w->d_x.reserve_exact(sizeof(float) * (size_t)longest * B));
    AF_HIP(w->d_tg.reserve_exact(sizeof(float) * (size_t)longest * B));
    w->scratch_frames = longest;
  }
  if (w->fresh) {
    AF_HIP(af::launch_output_writer_init(w->d_plane, B, stream));
    w->fresh = false;
  }
  af::OwPush p{};
  p.in = d_in;
  p.in_stride = in_stride;
  p.n = (int32_t)n_in;
  p.fill = d_fill;
  p.clean_path = clean_path ? 1 : 0;
  p.out = d_out;
  p.out_stride = out_stride;
  p.written = d_written;
  p.plane = w->d_plane;
  p.n_streams = B;
  p.x = w->d_x;
  p.tg = w->d_tg;
  p.max_out = (int32_t)max_out;
  p.limiter_on = w->limiter_enabled ? 1 : 0;
  p.ceiling = w->limiter_enabled ? w->ceiling_linear : 1.0f;                  // output_writer.rs:208-212
  p.limiter_ceiling = std::min(std::max(p.ceiling, 0.000001f), 1.0f);         // true_peak.rs:304-306
  p.clamp_ceiling = std::min(std::max(p.ceiling, 0.0f), 1.0f);                // routing.rs:774
  p.release_coeff = w->release_coeff;
  p.capacity = w->cfg.queue_capacity;
  p.center = w->cfg.target_center;
  p.hard = w->cfg.hard_backlog;
  p.fade = w->cfg.fade_frames;
  w->ev.restart();
  AF_HIP(w->ev.mark(stream));
  AF_HIP(af::launch_output_writer_plan(p, stream));
  AF_HIP(w->ev.mark(stream));
  AF_HIP(af::launch_output_writer_shape(p, stream));
  AF_HIP(w->ev.mark(stream));
  if (p.limiter_on) AF_HIP(af::launch_output_writer_gain(p, stream));
  AF_HIP(w->ev.mark(stream));
  AF_HIP(af::launch_output_writer_out(p, stream));
  AF_HIP(w->ev.mark(stream));
  AF_HIP(af::launch_output_writer_finish(p, stream));
  AF_HIP(w->ev.mark(stream));
  return AF_OK;
}

// rows [first, first + count) of the plane, or the fresh plane's values before a first push
int ow_read_rows(af_output_writer *w, int first, int count, std::vector<uint32_t> &rows) {
  const size_t B = (size_t)w->n_streams;
  rows.assign((size_t)count * B, 0u);
  if (w->d_plane && !w->fresh) {
    AF_HIP(hipSetDevice(w->device));
    AF_HIP(hipDeviceSynchronize());  // pushes may be queued on any stream
    AF_HIP(hipMemcpy(rows.data(), w->d_plane + (size_t)first * B, sizeof(uint32_t) * (size_t)count * B, hipMemcpyDeviceToHost));
    return AF_OK;
  }
  auto bits = [](float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; };
  for (int f = first; f < first + count; ++f) {
    float v = 0.0f;
    if (f == af::kOwGain || f == af::kOwMinGain || f == af::kOwRecRatio) v = 1.0f;
    if (f == af::kOwDbClipPeak || f == af::kOwDbTruePeak || f == af::kOwDbTruePeakInput) v = -120.0f;
    if (f == af::kOwDbHeadroom) v = 120.0f;
    for (size_t s = 0; s < B; ++s) rows[(size_t)(f - first) * B + s] = bits(v);
  }
  return AF_OK;
}

}  // namespace

extern "C" {

int af_output_writer_default_config(int32_t output_rate, af_output_writer_config *cfg) {
  if (!cfg) return fail(AF_ERR_INVALID_ARGUMENT, "cfg is null");
  if (output_rate <= 0) return fail(AF_ERR_INVALID_ARGUMENT, "output_rate must be positive");
  const int64_t low = ow_duration_samples(output_rate, 30), high = ow_duration_samples(output_rate, 40);  // processor.rs:66-67
  cfg->output_rate = output_rate;
  cfg->queue_capacity = 2 * (int64_t)output_rate;                          // dsp_loop.rs:204
  cfg->target_center = (low + high + 1) / 2;                               // dsp_loop.rs:786-787
  cfg->hard_backlog = ow_duration_samples(output_rate, 60);                // dsp_loop.rs:788-789, processor.rs:68
  cfg->fade_frames = std::max<int64_t>(ow_duration_samples(output_rate, 6), 1);  // dsp_loop.rs:794-795
  return AF_OK;
}

int af_output_writer_create(const af_output_writer_config *cfg, int32_t n_streams, int32_t device, af_output_writer **out) {
  if (!out) return fail(AF_ERR_INVALID_ARGUMENT, "out is null");
  *out = nullptr;
  if (!cfg) return fail(AF_ERR_INVALID_ARGUMENT, "cfg is null");
  constexpr int64_t kLim = INT32_MAX;
  if (cfg->output_rate <= 0) return fail(AF_ERR_INVALID_ARGUMENT, "output_rate must be positive");
  if (cfg->queue_capacity < 1 || cfg->queue_capacity > kLim) return fail(AF_ERR_INVALID_ARGUMENT, "queue_capacity must be 1 .. 2^31 - 1");
  if (cfg->target_center < 0 || cfg->target_center > kLim) return fail(AF_ERR_INVALID_ARGUMENT, "target_center must be 0 .. 2^31 - 1");
  if (cfg->hard_backlog < 0 || cfg->hard_backlog > kLim) return fail(AF_ERR_INVALID_ARGUMENT, "hard_backlog must be 0 .. 2^31 - 1");
  if (cfg->fade_frames < 1 || cfg->fade_frames > kLim) return fail(AF_ERR_INVALID_ARGUMENT, "fade_frames must be 1 .. 2^31 - 1");
  if (n_streams <= 0 || n_streams > 65535) return fail(AF_ERR_INVALID_ARGUMENT, "n_streams must be 1 .. 65535");
  if (device < 0) return fail(AF_ERR_INVALID_ARGUMENT, "device must be >= 0");
  af_output_writer *w = new af_output_writer();
  w->device = device;
  w->n_streams = n_streams;
  w->cfg = *cfg;
  const float rate = std::max((float)cfg->output_rate, 1.0f);  // true_peak.rs:279
  w->release_coeff = (float)af::time_constant_to_coeff((double)std::min(std::max(80.0f, 5.0f), 500.0f), (double)rate);
  *out = w;
  return AF_OK;
}

void af_output_writer_destroy(af_output_writer *w) { delete w; }

int af_output_writer_set_limiter(af_output_writer *w, int32_t enabled, float ceiling_linear) {
  if (!w) return fail(AF_ERR_INVALID_ARGUMENT, "output writer is null");
  if (!std::isfinite(ceiling_linear)) return fail(AF_ERR_INVALID_ARGUMENT, "ceiling_linear must be finite");
  w->limiter_enabled = enabled != 0;
  w->ceiling_linear = ceiling_linear;
  return AF_OK;
}

int af_output_writer_reset(af_output_writer *w) {
  if (!w) return fail(AF_ERR_INVALID_ARGUMENT, "output writer is null");
  w->fresh = true;  // the plane is rewritten in stream order in front of the next push
  return AF_OK;
}

int64_t af_output_writer_max_output_frames(const af_output_writer *w, int64_t n_in) {
  if (!w || n_in < 1) return 0;
  return ow_max_output_frames(w, n_in);
}

int af_output_writer_push_device(af_output_writer *w, const float *d_in, int64_t n_in, int64_t in_stride, const int64_t *d_fill,
                                 int32_t clean_path, float *d_out, int64_t out_capacity, int64_t out_stride, int64_t *d_written,
                                 void *hip_stream) {
  if (int rc = ow_push_check(w, d_in, n_in, in_stride, d_fill, d_out, out_capacity, out_stride, d_written)) return rc;
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  if (n_in == 0) {
    AF_HIP(hipSetDevice(w->device));
    AF_HIP(hipMemsetAsync(d_written, 0, sizeof(int64_t) * (size_t)w->n_streams, stream));
    return AF_OK;
  }
  return ow_enqueue(w, d_in, n_in, in_stride, d_fill, clean_path, d_out, out_stride, d_written, stream);
}

int af_output_writer_push_host(af_output_writer *w, const float *in, int64_t n_in, int64_t in_stride, const int64_t *fill,
                               int32_t clean_path, float *out, int64_t out_capacity, int64_t out_stride, int64_t *written) {
  if (int rc = ow_push_check(w, in, n_in, in_stride, fill, out, out_capacity, out_stride, written)) return rc;
  const int64_t B = w->n_streams;
  if (n_in == 0) {
    for (int64_t s = 0; s < B; ++s) written[s] = 0;
    return AF_OK;
  }
  for (int64_t s = 0; s < B; ++s)
    if (fill[s] < 0 || fill[s] > w->cfg.queue_capacity)
      return fail(AF_ERR_INVALID_ARGUMENT, "fill[%lld] = %lld is outside the queue's 0 .. %lld", (long long)s, (long long)fill[s],
                  (long long)w->cfg.queue_capacity);
  AF_HIP(hipSetDevice(w->device));
  const int64_t max_out = ow_max_output_frames(w, n_in);
  w->touched_device = true;
  AF_HIP(w->d_fill.reserve_exact(sizeof(int64_t) * (size_t)B));
  AF_HIP(w->d_written.reserve_exact(sizeof(int64_t) * (size_t)B));
  AF_HIP(w->d_in.reserve_exact(sizeof(float) * B * n_in));  // (the host entry point synchronises before it returns: nothing reads the old buffers)
  AF_HIP(w->d_out.reserve_exact(sizeof(float) * B * max_out));
  const size_t f4 = sizeof(float);
  AF_HIP(hipMemcpy2D(w->d_in, f4 * n_in, in, f4 * in_stride, f4 * n_in, B, hipMemcpyHostToDevice));
  AF_HIP(hipMemcpy(w->d_fill, fill, sizeof(int64_t) * (size_t)B, hipMemcpyHostToDevice));
  if (int rc = ow_enqueue(w, w->d_in, n_in, n_in, w->d_fill, clean_path, w->d_out, max_out, w->d_written, nullptr)) return rc;
  AF_HIP(hipStreamSynchronize(nullptr));
  AF_HIP(hipMemcpy(written, w->d_written, sizeof(int64_t) * (size_t)B, hipMemcpyDeviceToHost));
  int64_t longest = 0;
  for (int64_t s = 0; s < B; ++s) longest = std::max(longest, std::min(std::max<int64_t>(written[s], 0), max_out));
  if ((int64_t)w->host_rows.size() < B * longest) w->host_rows.resize((size_t)(B * longest));
  if (longest > 0)
    AF_HIP(hipMemcpy2D(w->host_rows.data(), f4 * longest, w->d_out, f4 * max_out, f4 * longest, B, hipMemcpyDeviceToHost));
  for (int64_t s = 0; s < B; ++s)  // the rest of a row stays as the caller left it
    std::memcpy(out + s * out_stride, w->host_rows.data() + s * longest, f4 * (size_t)std::min(std::max<int64_t>(written[s], 0), max_out));
  return AF_OK;
}

int af_output_writer_read_counters(af_output_writer *w, uint64_t *jitter_dropped, uint64_t *retime_adjustments,
                                   uint64_t *recovery_events, uint64_t *short_write_dropped, uint64_t *clip_events,
                                   uint64_t *true_peak_events, int32_t n_streams) {
  if (!w) return fail(AF_ERR_INVALID_ARGUMENT, "output writer is null");
  if (n_streams != w->n_streams) return fail(AF_ERR_INVALID_ARGUMENT, "n_streams must be the output writer's %d", w->n_streams);
  std::vector<uint32_t> rows;
  if (int rc = ow_read_rows(w, af::kOwCntJitterDropped, 12, rows)) return rc;
  static_assert(af::kOwCntTruePeak == af::kOwCntJitterDropped + 10, "the six counters are consecutive word pairs");
  const size_t B = (size_t)n_streams;
  uint64_t *dst[6] = {jitter_dropped, retime_adjustments, recovery_events, short_write_dropped, clip_events, true_peak_events};
  for (int c = 0; c < 6; ++c)
    if (dst[c])
      for (size_t s = 0; s < B; ++s) dst[c][s] = (uint64_t)rows[(2 * c) * B + s] | ((uint64_t)rows[(2 * c + 1) * B + s] << 32);
  return AF_OK;
}

int af_output_writer_read_meters(af_output_writer *w, float *db, float *linear, float *ratio, float *drift_ema, int64_t *out_len,
                                 int64_t *fade_remaining, int64_t *fill_after, int32_t n_streams) {
  if (!w) return fail(AF_ERR_INVALID_ARGUMENT, "output writer is null");
  if (n_streams != w->n_streams) return fail(AF_ERR_INVALID_ARGUMENT, "n_streams must be the output writer's %d", w->n_streams);
  std::vector<uint32_t> rows;
  if (int rc = ow_read_rows(w, 0, af::kOwCount, rows)) return rc;
  const size_t B = (size_t)n_streams;
  static_assert(af::kOwDbHeadroom == af::kOwDbClipPeak + 5 && af::kOwClipMax == af::kOwInTp + 4, "consecutive fields");
  if (db) std::memcpy(db, &rows[(size_t)af::kOwDbClipPeak * B], 4 * 6 * B);
  if (linear) std::memcpy(linear, &rows[(size_t)af::kOwInTp * B], 4 * 5 * B);
  if (ratio) std::memcpy(ratio, &rows[(size_t)af::kOwRecRatio * B], 4 * B);
  if (drift_ema) std::memcpy(drift_ema, &rows[(size_t)af::kOwEma * B], 4 * B);
  for (size_t s = 0; s < B; ++s) {
    if (out_len) out_len[s] = rows[(size_t)af::kOwRecOutLen * B + s];
    if (fade_remaining) fade_remaining[s] = rows[(size_t)af::kOwFadeRemaining * B + s];
    if (fill_after) fill_after[s] = rows[(size_t)af::kOwRecFillAfter * B + s];
  }
  return AF_OK;
}

int af_output_writer_read_state(af_output_writer *w, float *gain, float *delay, int32_t *write_idx, float *histories,
                                int32_t n_streams) {
  if (!w) return fail(AF_ERR_INVALID_ARGUMENT, "output writer is null");
  if (n_streams != w->n_streams) return fail(AF_ERR_INVALID_ARGUMENT, "n_streams must be the output writer's %d", w->n_streams);
  std::vector<uint32_t> rows;
  if (int rc = ow_read_rows(w, 0, af::kOwCount, rows)) return rc;
  const size_t B = (size_t)n_streams;
  auto at = [&](int f, size_t s) { float v; std::memcpy(&v, &rows[(size_t)f * B + s], 4); return v; };
  for (size_t s = 0; s < B; ++s) {
    const int sel = (int)(rows[(size_t)af::kOwSel * B + s] & 1u);
    const int base = af::kOwHist + sel * 3 * af::kOwTaps;
    const int widx = (int)rows[(size_t)af::kOwWriteIdx * B + s];
    if (gain) gain[s] = at(af::kOwGain, s);
    if (write_idx) write_idx[s] = widx;
    if (histories)
      for (int k = 0; k < 3 * af::kOwTaps; ++k) histories[s * 3 * af::kOwTaps + k] = at(base + k, s);
    if (delay)  // the frame k + 1 steps back sits k + 1 slots behind the write index (true_peak.rs:343-345)
      for (int k = 0; k < af::kOwLookahead; ++k)
        delay[s * af::kOwLookahead + (size_t)((widx - 1 - k + 2 * af::kOwLookahead) % af::kOwLookahead)] = at(base + k, s);
  }
  return AF_OK;
}

int af_output_writer_last_kernel_ms(af_output_writer *w, double *ms) {
  if (!w) return fail(AF_ERR_INVALID_ARGUMENT, "output writer is null");
  if (ms) *ms = 0.0;
  if (!w->timed()) return AF_OK;
  AF_HIP(hipSetDevice(w->device));
  AF_HIP(w->ev.wait_last());
  double t = 0.0;
  AF_HIP(w->ev.elapsed(0, 5, &t));
  if (ms) *ms = t;
  return AF_OK;
}

int af_output_writer_last_pass_ms(af_output_writer *w, double *pass_ms) {
  if (!w || !pass_ms) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  for (int k = 0; k < 5; ++k) pass_ms[k] = 0.0;
  if (!w->timed()) return AF_OK;
  AF_HIP(hipSetDevice(w->device));
  AF_HIP(w->ev.wait_last());
  for (int k = 0; k < 5; ++k) AF_HIP(w->ev.elapsed(k, k + 1, &pass_ms[k]));
  return AF_OK;
}

}  // extern "C"
