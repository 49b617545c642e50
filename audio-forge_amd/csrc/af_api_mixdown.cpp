// af_api_mixdown.cpp -- the C ABI of the input mixdown (af_mixdown_*).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "af_api_internal.hpp"
#include "af_mixdown_host.hpp"

// ------------------------------------------------------------------------------------------
// The capture callback's mixdown (input.rs:383-736, 785-843): interleaved device frames -> mono.  Kernels, passes and the
// state plane: af_mixdown.hip / af_mixdown_host.hpp.
struct af_mixdown {
  int device = 0, n_streams = 0, channels = 1;
  int mode = 0;               // live: read at each push, per chunk (input.rs:814-816)
  bool fresh = true;          // the plane is (re)initialised in stream order in front of the next push
  bool touched_device = false;  // a push allocated (or may have): the destructor has a device to wait for
  af::DeviceBuffer<uint32_t> d_plane;
  af::DeviceBuffer<float> d_in, d_out;  // staging of the host entry point
  af::EventChain events;      // three marks per chunk of the last push: before the decision pass | between | after the mix
  int timed_chunks = 0;
  ~af_mixdown() {  // the device comes to rest before the members release themselves
    if (touched_device) { (void)hipSetDevice(device); (void)hipDeviceSynchronize(); }
  }
};

namespace {

int mixdown_check_mode(int32_t mode) {
  if (mode < 0 || mode > 4)
    return fail(AF_ERR_INVALID_ARGUMENT, "unknown input channel mode %d (0 average, 1 left, 2 right, 3 max_rms, 4 phase_safe_mono)", mode);
  return AF_OK;
}

int mixdown_push_check(af_mixdown *m, const float *in, int64_t n_frames, int64_t in_stride, const float *out, int64_t out_stride) {
  if (!m) return fail(AF_ERR_INVALID_ARGUMENT, "mixdown is null");
  if (n_frames < 0 || in_stride < n_frames) return fail(AF_ERR_INVALID_ARGUMENT, "in_stride must cover n_frames frames");
  if (out_stride < n_frames) return fail(AF_ERR_INVALID_ARGUMENT, "out_stride must cover n_frames frames");
  if ((!in || !out) && n_frames > 0) return fail(AF_ERR_INVALID_ARGUMENT, "null buffer");
  return AF_OK;
}

// one callback (input.rs:807-842): chunks of at most 8192 frames, one decision per chunk, all enqueued on `stream`
int mixdown_enqueue(af_mixdown *m, const float *d_in, int64_t n_frames, int64_t in_stride, float *d_out, int64_t out_stride,
                    hipStream_t stream) {
  AF_HIP(hipSetDevice(m->device));
  m->touched_device = true;
  if (!m->d_plane) {
    AF_HIP(m->d_plane.reserve_exact(sizeof(uint32_t) * af::kMfCount * (size_t)m->n_streams));
    m->fresh = true;
  }
  if (m->fresh) {
    AF_HIP(af::launch_mixdown_init(m->d_plane, m->n_streams, stream));
    m->fresh = false;
  }
  const int C = m->channels, mode = m->mode, B = m->n_streams;
  const int64_t chunks = (n_frames + af::kMixChunk - 1) / af::kMixChunk;
  m->events.restart();
  m->timed_chunks = 0;
  for (int64_t j = 0; j < chunks; ++j) {
    const int64_t at = j * af::kMixChunk;
    const int32_t n = (int32_t)std::min<int64_t>(af::kMixChunk, n_frames - at);
    const float *src = d_in + at * C;
    float *dst = d_out + at;
    int host_kind = -1, host_channel = 0;
    AF_HIP(m->events.mark(stream));
    if (C == 2) {  // stereo always gets its correlation and warning count (input.rs:675-677, 833-838)
      AF_HIP(af::launch_mixdown_decide(src, in_stride, n, m->d_plane, B, mode, stream));
    } else if (C > 2 && mode == af::kMixMaxRms) {
      AF_HIP(af::launch_mixdown_energy(src, in_stride, n, C, m->d_plane, B, stream));
    } else if (C == 1) {  // the one-channel copy, input.rs:789-805
      host_kind = af::kMixKindSelect;
    } else if (mode == af::kMixLeft || mode == af::kMixRight) {
      host_kind = af::kMixKindSelect;
      host_channel = mode == af::kMixRight ? 1 : 0;
    } else {  // Average, and PhaseSafeMono off stereo (input.rs:719)
      host_kind = af::kMixKindAverage;
    }
    AF_HIP(m->events.mark(stream));
    AF_HIP(af::launch_mixdown_mix(src, in_stride, n, C, dst, out_stride, m->d_plane, B, host_kind, host_channel, stream));
    AF_HIP(m->events.mark(stream));
  }
  m->timed_chunks = (int)chunks;
  return AF_OK;
}

}  // namespace

extern "C" {

int af_mixdown_create(int32_t n_channels, int32_t mode, int32_t n_streams, int32_t device, af_mixdown **out) {
  if (!out) return fail(AF_ERR_INVALID_ARGUMENT, "out is null");
  *out = nullptr;
  if (n_channels < 1) return fail(AF_ERR_INVALID_ARGUMENT, "n_channels must be >= 1");
  if (n_channels > af::kMixMaxChannels)
    return fail(AF_ERR_UNSUPPORTED, "%d input channels: the mixdown is built for at most %d", n_channels, af::kMixMaxChannels);
  if (int rc = mixdown_check_mode(mode)) return rc;
  if (n_streams <= 0) return fail(AF_ERR_INVALID_ARGUMENT, "n_streams must be positive");
  if (device < 0) return fail(AF_ERR_INVALID_ARGUMENT, "device must be >= 0");
  af_mixdown *m = new af_mixdown();
  m->device = device;
  m->n_streams = n_streams;
  m->channels = n_channels;
  m->mode = mode;
  *out = m;
  return AF_OK;
}

void af_mixdown_destroy(af_mixdown *m) { delete m; }

int af_mixdown_set_mode(af_mixdown *m, int32_t mode) {
  if (!m) return fail(AF_ERR_INVALID_ARGUMENT, "mixdown is null");
  if (int rc = mixdown_check_mode(mode)) return rc;
  m->mode = mode;
  return AF_OK;
}

int32_t af_mixdown_mode(const af_mixdown *m) { return m ? m->mode : 0; }
int32_t af_mixdown_channels(const af_mixdown *m) { return m ? m->channels : 0; }

int af_mixdown_reset(af_mixdown *m) {
  if (!m) return fail(AF_ERR_INVALID_ARGUMENT, "mixdown is null");
  m->fresh = true;  // the plane is rewritten in stream order in front of the next push
  return AF_OK;
}

int af_mixdown_push_device(af_mixdown *m, const float *d_in, int64_t n_frames, int64_t in_stride_frames, float *d_out,
                           int64_t out_stride, void *hip_stream) {
  if (int rc = mixdown_push_check(m, d_in, n_frames, in_stride_frames, d_out, out_stride)) return rc;
  if (n_frames == 0) return AF_OK;
  return mixdown_enqueue(m, d_in, n_frames, in_stride_frames, d_out, out_stride, static_cast<hipStream_t>(hip_stream));
}

int af_mixdown_push_host(af_mixdown *m, const float *in, int64_t n_frames, int64_t in_stride_frames, float *out, int64_t out_stride) {
  if (int rc = mixdown_push_check(m, in, n_frames, in_stride_frames, out, out_stride)) return rc;
  const int64_t B = m->n_streams, C = m->channels;
  if (!af::check_finite(in, B, n_frames * C, in_stride_frames * C)) return fail(AF_ERR_NON_FINITE, "samples must be finite");
  if (n_frames == 0) return AF_OK;
  AF_HIP(hipSetDevice(m->device));
  m->touched_device = true;
  AF_HIP(m->d_in.reserve_exact(sizeof(float) * B * n_frames * C));  // (the host entry point synchronises before it returns: nothing reads the old buffers)
  AF_HIP(m->d_out.reserve_exact(sizeof(float) * B * n_frames));
  const size_t f4 = sizeof(float);
  AF_HIP(hipMemcpy2D(m->d_in, f4 * n_frames * C, in, f4 * in_stride_frames * C, f4 * n_frames * C, B, hipMemcpyHostToDevice));
  if (int rc = mixdown_enqueue(m, m->d_in, n_frames, n_frames, m->d_out, n_frames, nullptr)) return rc;
  AF_HIP(hipStreamSynchronize(nullptr));
  AF_HIP(hipMemcpy2D(out, f4 * out_stride, m->d_out, f4 * n_frames, f4 * n_frames, B, hipMemcpyDeviceToHost));
  return AF_OK;
}

int af_mixdown_read_diagnostics(af_mixdown *m, float *stereo_correlation, uint64_t *phase_warning_count, int32_t *strategy,
                                float *estimated_delay, int32_t *polarity_flipped, int32_t n_streams) {
  if (!m) return fail(AF_ERR_INVALID_ARGUMENT, "mixdown is null");
  if (n_streams != m->n_streams) return fail(AF_ERR_INVALID_ARGUMENT, "n_streams must be the mixdown's %d", m->n_streams);
  const size_t B = (size_t)n_streams;
  std::vector<uint32_t> rows(6 * B, 0u);
  if (m->d_plane && !m->fresh) {
    AF_HIP(hipSetDevice(m->device));
    AF_HIP(hipDeviceSynchronize());  // pushes may be queued on any stream
    AF_HIP(hipMemcpy(rows.data(), m->d_plane + (size_t)af::kMfDiagCorrelation * B, sizeof(uint32_t) * 6 * B, hipMemcpyDeviceToHost));
  } else {
    for (size_t s = 0; s < B; ++s) rows[s] = 0x7fc00000u;  // no Some yet
  }
  static_assert(af::kMfDiagFlipped == af::kMfDiagCorrelation + 5, "the six diagnostic fields are consecutive");
  for (size_t s = 0; s < B; ++s) {
    if (stereo_correlation) std::memcpy(&stereo_correlation[s], &rows[s], 4);
    if (phase_warning_count) phase_warning_count[s] = (uint64_t)rows[B + s] | ((uint64_t)rows[2 * B + s] << 32);
    if (strategy) strategy[s] = (int32_t)rows[3 * B + s];
    if (estimated_delay) std::memcpy(&estimated_delay[s], &rows[4 * B + s], 4);
    if (polarity_flipped) polarity_flipped[s] = (int32_t)rows[5 * B + s];
  }
  return AF_OK;
}

int af_mixdown_last_kernel_ms(af_mixdown *m, double *decision_ms, double *mix_ms) {
  if (!m) return fail(AF_ERR_INVALID_ARGUMENT, "mixdown is null");
  if (decision_ms) *decision_ms = 0.0;
  if (mix_ms) *mix_ms = 0.0;
  if (m->timed_chunks == 0) return AF_OK;
  AF_HIP(hipSetDevice(m->device));
  AF_HIP(m->events.wait_last());
  for (size_t j = 0; j < (size_t)m->timed_chunks; ++j) {
    double a = 0.0, b = 0.0;
    AF_HIP(m->events.elapsed(3 * j, 3 * j + 1, &a));
    AF_HIP(m->events.elapsed(3 * j + 1, 3 * j + 2, &b));
    if (decision_ms) *decision_ms += a;
    if (mix_ms) *mix_ms += b;
  }
  return AF_OK;
}

}  // extern "C"
