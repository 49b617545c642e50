// af_api_noise_suppressor.cpp -- the C ABI of the NoiseSuppressor wrapper (af_noise_model_*, af_noise_suppressor_*).  It holds
// an engine and talks to it through include/audioforge_mi.h and af_engine_reinit_suppressor_state (af_api_internal.hpp).
#include <algorithm>
#include <cctype>
#include <cstring>
#include <string>
#include <vector>

#include "af_api_internal.hpp"
#include "af_suppressor.h"

// ------------------------------------------------------------------------------------------
// NoiseSuppressor (rust-core/src/dsp/noise_suppressor.rs:89-194) for a batch of streams: the trait's ring surface over an
// engine that runs the suppressor alone.  All streams advance in lock step, so the two fixed rings of
// RNNoiseProcessor (rnnoise.rs:11,27-28; audio/rt.rs:146-248) are one pair of [stream][capacity] host buffers with shared
// counters; whole frames go through the GPU in one call per process_frames().
struct af_noise_suppressor {
  af_engine *engine = nullptr;
  int32_t model = AF_NOISE_MODEL_RNNOISE;
  int32_t n_streams = 0;
  bool enabled = true;  // rnnoise.rs:58
  float strength = 1.0f;
  std::vector<float> in_ring, out_ring;  // [stream][kCapacity], linear (compacted on pop)
  int64_t in_len = 0, out_len = 0;
  std::vector<float> scratch_in, scratch_out;
  static constexpr int64_t kCapacity = 8192 + af::kRnnFrame;  // RNNOISE_BUFFER_CAPACITY, rnnoise.rs:11
};

extern "C" {

int af_noise_model_from_id(const char *id, int32_t *model) {  // NoiseModel::from_id, noise_suppressor.rs:58-67
  if (!id || !model) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  std::string lower(id);
  for (char &c : lower) c = (char)std::tolower((unsigned char)c);
  if (lower == "rnnoise") { *model = AF_NOISE_MODEL_RNNOISE; return AF_OK; }
  if (lower == "deepfilter-ll" || lower == "deepfilterll") { *model = AF_NOISE_MODEL_DEEPFILTER_LL; return AF_OK; }
  if (lower == "deepfilter" || lower == "deepfilternet") { *model = AF_NOISE_MODEL_DEEPFILTER; return AF_OK; }
  return fail(AF_ERR_INVALID_ARGUMENT, "unknown noise model id '%s'", id);
}
const char *af_noise_model_id(int32_t model) {  // noise_suppressor.rs:47-55
  switch (model) {
    case AF_NOISE_MODEL_RNNOISE: return "rnnoise";
    case AF_NOISE_MODEL_DEEPFILTER_LL: return "deepfilter-ll";
    case AF_NOISE_MODEL_DEEPFILTER: return "deepfilter";
    default: return "";
  }
}
const char *af_noise_model_display_name(int32_t model) {  // noise_suppressor.rs:36-44
  switch (model) {
    case AF_NOISE_MODEL_RNNOISE: return "RNNoise (Low Latency)";
    case AF_NOISE_MODEL_DEEPFILTER_LL: return "DeepFilterNet LL (Fast)";
    case AF_NOISE_MODEL_DEEPFILTER: return "DeepFilterNet (Best Quality)";
    default: return "";
  }
}
int32_t af_noise_model_available(int32_t *models, int32_t capacity) {  // NoiseModel::available, noise_suppressor.rs:70-84
  // the DeepFilterNet variants exist in the reference only behind its `deepfilter` feature and a runtime-loaded df library +
  // model archives; neither is built here, so the list is what a default build of the reference returns
  if (models && capacity > 0) models[0] = AF_NOISE_MODEL_RNNOISE;
  return 1;
}

int af_noise_suppressor_create(int32_t model, int32_t n_streams, int32_t device, af_noise_suppressor **out) {
  if (!out) return fail(AF_ERR_INVALID_ARGUMENT, "out is null");
  *out = nullptr;
  if (model == AF_NOISE_MODEL_DEEPFILTER_LL || model == AF_NOISE_MODEL_DEEPFILTER)
    return fail(AF_ERR_UNSUPPORTED, "the DeepFilterNet backend is not built: its model archives and runtime library are not "
                                    "part of the reference checkout (deepfilter_ffi.rs:9-16); use 'rnnoise'");
  if (model != AF_NOISE_MODEL_RNNOISE) return fail(AF_ERR_INVALID_ARGUMENT, "unknown noise model %d", model);
  af_engine *e = nullptr;
  if (int rc = af_engine_create(48000.0, n_streams, device, &e)) return rc;
  int rc = af_engine_set_eq_enabled(e, 0);
  if (!rc) rc = af_engine_set_compressor_enabled(e, 0);
  if (!rc) rc = af_engine_set_limiter_enabled(e, 0);
  if (!rc) rc = af_engine_set_input_scrub_enabled(e, 0);  // scale_sample_for_model zeroes non-finite model input itself (rnnoise.rs:90-93)
  if (!rc) rc = af_engine_set_control_block_samples(e, af::kRnnFrame);
  if (!rc) rc = af_engine_set_suppressor_enabled(e, 1);
  if (rc) {
    af_engine_destroy(e);
    return rc;
  }
  af_noise_suppressor *s = new af_noise_suppressor();
  s->engine = e;
  s->model = model;
  s->n_streams = n_streams;
  s->in_ring.assign((size_t)n_streams * af_noise_suppressor::kCapacity, 0.0f);
  s->out_ring.assign((size_t)n_streams * af_noise_suppressor::kCapacity, 0.0f);
  *out = s;
  return AF_OK;
}
void af_noise_suppressor_destroy(af_noise_suppressor *s) {
  if (!s) return;
  af_engine_destroy(s->engine);
  delete s;
}
af_engine *af_noise_suppressor_engine(af_noise_suppressor *s) { return s ? s->engine : nullptr; }

// push_samples: `samples` is [stream][stride]; returns how many samples per stream the fixed input ring accepted
int64_t af_noise_suppressor_push_samples(af_noise_suppressor *s, const float *samples, int64_t n, int64_t stride) {
  if (!s || (!samples && n > 0) || n < 0 || stride < n) return fail(AF_ERR_INVALID_ARGUMENT, "bad push_samples arguments");
  const int64_t cap = af_noise_suppressor::kCapacity;
  const int64_t written = std::min<int64_t>(n, cap - s->in_len);  // FixedAudioRing::push_slice, rt.rs:189-197
  for (int32_t k = 0; k < s->n_streams; ++k)
    std::memcpy(&s->in_ring[(size_t)k * cap + s->in_len], samples + (size_t)k * stride, sizeof(float) * written);
  s->in_len += written;
  return written;
}

static void ring_consume(std::vector<float> &ring, int64_t &len, int64_t count, int32_t n_streams) {
  const int64_t cap = af_noise_suppressor::kCapacity;
  if (count <= 0) return;
  for (int32_t k = 0; k < n_streams; ++k)
    std::memmove(&ring[(size_t)k * cap], &ring[(size_t)k * cap + count], sizeof(float) * (len - count));
  len -= count;
}

int af_noise_suppressor_process_frames(af_noise_suppressor *s) {  // rnnoise.rs:122-164
  if (!s) return fail(AF_ERR_INVALID_ARGUMENT, "suppressor is null");
  const int64_t cap = af_noise_suppressor::kCapacity;
  if (!s->enabled) {  // bypass: input_buffer.move_into(&mut output_buffer), rnnoise.rs:123-126
    const int64_t moved = std::min<int64_t>(s->in_len, cap - s->out_len);
    for (int32_t k = 0; k < s->n_streams; ++k)
      std::memcpy(&s->out_ring[(size_t)k * cap + s->out_len], &s->in_ring[(size_t)k * cap], sizeof(float) * moved);
    s->out_len += moved;
    ring_consume(s->in_ring, s->in_len, moved, s->n_streams);
    return AF_OK;
  }
  // while input.len() >= 480 && output.remaining() >= 480
  const int64_t frames = std::min<int64_t>(s->in_len / af::kRnnFrame, (cap - s->out_len) / af::kRnnFrame);
  if (frames <= 0) return AF_OK;
  const int64_t n = frames * af::kRnnFrame;
  s->scratch_in.resize((size_t)s->n_streams * n);
  s->scratch_out.resize((size_t)s->n_streams * n);
  for (int32_t k = 0; k < s->n_streams; ++k)
    std::memcpy(&s->scratch_in[(size_t)k * n], &s->in_ring[(size_t)k * cap], sizeof(float) * n);
  if (int rc = af_engine_set_suppressor_strength(s->engine, s->strength)) return rc;
  if (int rc = af_engine_process_host(s->engine, s->scratch_in.data(), s->scratch_out.data(), n, AF_LAYOUT_STREAM_MAJOR)) return rc;
  for (int32_t k = 0; k < s->n_streams; ++k)
    std::memcpy(&s->out_ring[(size_t)k * cap + s->out_len], &s->scratch_out[(size_t)k * n], sizeof(float) * n);
  s->out_len += n;
  ring_consume(s->in_ring, s->in_len, n, s->n_streams);
  return AF_OK;
}

int64_t af_noise_suppressor_available_samples(const af_noise_suppressor *s) { return s ? s->out_len : 0; }
int64_t af_noise_suppressor_pending_input(const af_noise_suppressor *s) { return s ? s->in_len : 0; }

// pop_samples_into / read_samples (rnnoise.rs:185-188): up to `count` samples per stream into out[stream][stride]
int64_t af_noise_suppressor_pop_samples_into(af_noise_suppressor *s, float *out, int64_t count, int64_t stride) {
  if (!s || (!out && count > 0) || count < 0 || stride < count) return fail(AF_ERR_INVALID_ARGUMENT, "bad pop_samples_into arguments");
  const int64_t cap = af_noise_suppressor::kCapacity;
  const int64_t n = std::min<int64_t>(count, s->out_len);
  for (int32_t k = 0; k < s->n_streams; ++k) std::memcpy(out + (size_t)k * stride, &s->out_ring[(size_t)k * cap], sizeof(float) * n);
  ring_consume(s->out_ring, s->out_len, n, s->n_streams);
  return n;
}
int64_t af_noise_suppressor_drain_pending_input(af_noise_suppressor *s, float *out, int64_t capacity, int64_t stride) {  // rnnoise.rs:240-244
  if (!s || (!out && capacity > 0) || capacity < 0 || stride < capacity) return fail(AF_ERR_INVALID_ARGUMENT, "bad drain_pending_input arguments");
  const int64_t cap = af_noise_suppressor::kCapacity;
  const int64_t n = std::min<int64_t>(capacity, s->in_len);
  for (int32_t k = 0; k < s->n_streams; ++k) std::memcpy(out + (size_t)k * stride, &s->in_ring[(size_t)k * cap], sizeof(float) * n);
  ring_consume(s->in_ring, s->in_len, n, s->n_streams);
  return n;
}

int af_noise_suppressor_set_strength(af_noise_suppressor *s, float value) {  // rnnoise.rs:67-72
  if (!s) return fail(AF_ERR_INVALID_ARGUMENT, "suppressor is null");
  s->strength = value < 0.0f ? 0.0f : (value > 1.0f ? 1.0f : value);
  return AF_OK;
}
float af_noise_suppressor_get_strength(const af_noise_suppressor *s) { return s ? s->strength : 0.0f; }
int af_noise_suppressor_set_enabled(af_noise_suppressor *s, int32_t enabled) {  // rnnoise.rs:194-196: state is kept
  if (!s) return fail(AF_ERR_INVALID_ARGUMENT, "suppressor is null");
  s->enabled = enabled != 0;
  return AF_OK;
}
int32_t af_noise_suppressor_is_enabled(const af_noise_suppressor *s) { return s && s->enabled ? 1 : 0; }
int af_noise_suppressor_soft_reset(af_noise_suppressor *s) {  // flush_buffers, rnnoise.rs:216-232: model state survives
  if (!s) return fail(AF_ERR_INVALID_ARGUMENT, "suppressor is null");
  s->in_len = s->out_len = 0;
  return AF_OK;
}
int af_noise_suppressor_reset(af_noise_suppressor *s) {  // rnnoise.rs:205-210: a new DenoiseState + empty rings
  if (!s) return fail(AF_ERR_INVALID_ARGUMENT, "suppressor is null");
  s->in_len = s->out_len = 0;
  return af_engine_reinit_suppressor_state(s->engine);
}
int32_t af_noise_suppressor_model_type(const af_noise_suppressor *s) { return s ? s->model : -1; }
int32_t af_noise_suppressor_latency_samples(const af_noise_suppressor *) { return af::kRnnFrame; }  // rnnoise.rs:313-315
int32_t af_noise_suppressor_backend_available(const af_noise_suppressor *s) { return s ? 1 : 0; }   // rnnoise.rs:317-319
int32_t af_noise_suppressor_backend_failed(const af_noise_suppressor *) { return 0; }               // rnnoise.rs:325-327
const char *af_noise_suppressor_backend_error(const af_noise_suppressor *) { return nullptr; }      // rnnoise.rs:321-323

}  // extern "C"
