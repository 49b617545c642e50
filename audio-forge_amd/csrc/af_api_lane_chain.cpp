// af_api_lane_chain.cpp -- the C ABI of the streaming lane chain (af_lane_chain_*): one processor per stream, each under its own
// settings (python/mic_eq/config_parts/settings.py:543-593).  The kernels are af_lane_chain.hip's; every stream's parameters
// and starting state come from the host mirror of the reference's setters (af_host.hpp), which the engine uses too, replayed
// per stream in python_api.rs:400-487's order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "af_api_internal.hpp"
#include "af_host.hpp"
#include "af_lane_chain_host.hpp"

struct af_lane_chain {
  int device = 0;
  double sample_rate = 48000.0, lookahead_ms = 2.0;
  int32_t n_streams = 0, lanes_padded = 0, lookahead_samples = 96, control_block = 960;
  bool touched_device = false;
  // host side: what every stream was last configured with, and what has not reached the device yet
  std::vector<af_lane_chain_settings> settings;  // [n_streams]
  std::vector<uint8_t> configured;               // [n_streams]: 0 = OfflineDspBlockProcessor's defaults
  std::vector<uint8_t> dirty;                    // [lanes_padded]
  std::vector<int64_t> processed;                // [n_streams] since the stream's last configure / reset
  int64_t samples_total = 0;                     // processed by the object: the phase of the rings
  af::CompressorParams uniform{};
  // device side
  af::DeviceBuffer<double> d_p64, d_col64;
  af::DeviceBuffer<uint32_t> d_p32, d_col32;
  af::DeviceBuffer<int32_t> d_streams;
  af::DeviceBuffer<float> d_in, d_out;
  af::DeviceBuffer<af::BlockStats> d_rows;
  std::vector<double> col64;  // the columns of a flush, rewritten by the next one: they leave through pinned slots
  std::vector<uint32_t> col32;
  std::vector<int32_t> col_streams;
  af::PinnedSlots<6> slots;  // two flushes of three uploads in flight before a slot is used again
  // the last call
  int64_t blocks = 0;
  hipStream_t last_stream = nullptr;
  af::TimedSpan span;

  ~af_lane_chain();
};

namespace {

// The object's device for the length of a call; the caller's current device is put back afterwards.
class DeviceScope {
 public:
  explicit DeviceScope(int device) {
    if (hipGetDevice(&previous_) != hipSuccess) previous_ = -1;
    status_ = hipSetDevice(device);
  }
  ~DeviceScope() {
    if (previous_ >= 0) (void)hipSetDevice(previous_);
  }
  DeviceScope(const DeviceScope &) = delete;
  DeviceScope &operator=(const DeviceScope &) = delete;
  hipError_t status() const { return status_; }

 private:
  int previous_ = -1;
  hipError_t status_ = hipSuccess;
};

}  // namespace

af_lane_chain::~af_lane_chain() {
  if (!touched_device) return;
  DeviceScope scope(device);
  (void)hipDeviceSynchronize();
}

static_assert(sizeof(af::BlockStats) == sizeof(af_block_stats), "the kernel writes af_block_stats rows");

namespace {

uint32_t f32_bits(float v) {
  uint32_t u;
  std::memcpy(&u, &v, sizeof u);
  return u;
}

// One stream's column: OfflineDspBlockProcessor::new (block_processor.rs:31-60) and, for a configured stream, the setters in
// python_api.rs:400-487's order.  `st` null: the processor's defaults.
void lc_column(const af_lane_chain *h, const af_lane_chain_settings *st, double *c64, uint32_t *c32) {
  af::ChainProto p(h->sample_rate);
  p.limiter.set_lookahead_ms(h->lookahead_ms);
  if (st) {
    p.eq_enabled = true;
    for (int i = 0; i < af::kNumBands; ++i) {
      p.eq.set_band_frequency(i, st->bands[i][0]);
      p.eq.set_band_gain(i, st->bands[i][1]);
      p.eq.set_band_q(i, st->bands[i][2]);
    }
    p.eq_enabled = st->eq_enabled != 0;  // (simulate_auto_eq_chain has no such key: the processor's own switch, applied last)
    p.compressor_enabled = st->compressor_enabled != 0;
    if (p.compressor_enabled) {
      p.compressor.set_threshold(st->compressor_threshold_db);
      p.compressor.set_ratio(st->compressor_ratio);
      p.compressor.set_attack_time(st->compressor_attack_ms);
      p.compressor.set_release_time(st->compressor_release_ms);
      p.compressor.set_makeup_gain(st->compressor_makeup_gain_db);
      p.compressor.set_adaptive_release(st->compressor_adaptive_release != 0);
      p.compressor.set_base_release_time(st->compressor_base_release_ms);
      p.compressor.set_auto_makeup_enabled(false);
      p.compressor.set_sidechain_highpass_enabled(st->compressor_sidechain_highpass_enabled != 0);
    }
    p.limiter_enabled = st->limiter_enabled != 0;
    if (p.limiter_enabled) {
      // effective_limiter_ceiling_db, control.rs:904-910, then `as f32`
      const float effective =
          (float)(st->limiter_careful_output_enabled ? std::fmin(st->limiter_ceiling_db, -1.5) : st->limiter_ceiling_db);
      p.limiter.set_ceiling((double)effective);
      p.limiter.set_release_time(st->limiter_release_ms);
      p.tp_limiter.set_release_ms((float)st->limiter_release_ms);
    }
  }
  std::fill(c64, c64 + af::kLcF64Rows, 0.0);
  std::fill(c32, c32 + af::kLcF32Fixed, 0u);
  for (int k = 0; k < af::kNumBands; ++k) {  // a legacy (frequency, gain, Q) band is always one section
    const af::SectionParams sp = p.eq.bands[k].sections[0].section();
    const double v[10] = {sp.active.b0,  sp.active.b1,  sp.active.b2,  sp.active.a1,  sp.active.a2,
                          sp.pending.b0, sp.pending.b1, sp.pending.b2, sp.pending.a1, sp.pending.a2};
    std::copy(v, v + 10, c64 + af::kLcCoef + 10 * k);
    c32[af::kLcFade + 2 * k] = (uint32_t)sp.xf_total;
    c32[af::kLcFade + 2 * k + 1] = (uint32_t)sp.xf_remaining;
  }
  // a fresh compressor: af_api.cpp, initial_rows
  const af::CompressorProto &c = p.compressor;
  double *cs = c64 + af::kLcComp;  // DynCompState's order
  cs[6] = -120.0;                  // peak_env_db
  cs[8] = c.current_gain_reduction_db;
  cs[9] = c.fast_release_env_db;
  cs[10] = c.slow_release_env_db;
  cs[11] = c.current_release_ms;
  cs[12] = c.target_release_ms;
  cs[13] = af::time_constant_to_coeff(c.current_release_ms, c.sample_rate);  // compressor.rs:760-761
  cs[14] = c.smoothed_makeup_gain;
  c64[af::kLcLimGain] = 1.0;
  const af::CompressorParams q = c.params(h->control_block);
  c64[af::kLcThresholdDb] = q.threshold_db;
  c64[af::kLcAttackCoeff] = q.attack_coeff;
  c64[af::kLcDetectorReleaseCoeff] = q.detector_release_coeff;
  c64[af::kLcBaseReleaseMs] = q.base_release_ms;
  c64[af::kLcMakeupGainDb] = q.makeup_gain_db;
  c64[af::kLcCompFactor] = q.comp_factor;
  c64[af::kLcKneeStart] = q.knee_start;
  c64[af::kLcKneeEnd] = q.knee_end;
  const af::LimiterParams lp = p.limiter.params();
  c64[af::kLcLimCeilingLinear] = lp.ceiling_linear;
  c64[af::kLcLimReleaseCoeff] = lp.release_coeff;
  // block_processor.rs:150-151: the TP ceiling follows the limiter ceiling on every block
  af::TruePeakProto tp = p.tp_limiter;
  tp.set_ceiling_linear(std::pow(10.0f, (float)p.limiter.ceiling_db / 20.0f));
  c32[af::kLcTpCeiling] = f32_bits(tp.ceiling_linear);
  c32[af::kLcTpReleaseCoeff] = f32_bits(tp.release_coeff);
  c32[af::kLcTpGain] = f32_bits(1.0f);
  c32[af::kLcFlags] = (p.eq_enabled ? af::kLcEqOn : 0u) | (p.compressor_enabled ? af::kLcCompressorOn : 0u) |
                      (p.limiter_enabled ? af::kLcLimiterOn : 0u) | (q.adaptive_release ? af::kLcAdaptiveRelease : 0u) |
                      (q.sidechain_highpass_enabled ? af::kLcSidechainHighpass : 0u);
}

// The planes exist and every dirty lane's column is on its way, in `q`'s order before the next kernel.
int lc_flush(af_lane_chain *h, hipStream_t q) {
  const int64_t LP = h->lanes_padded;
  const int f32_rows = af::lc_f32_rows(h->lookahead_samples);
  if (!h->d_p64.get()) {
    AF_HIP(h->d_p64.reserve_exact(sizeof(double) * (size_t)af::kLcF64Rows * LP));
    AF_HIP(h->d_p32.reserve_exact(sizeof(uint32_t) * (size_t)f32_rows * LP));
  }
  h->col_streams.clear();
  for (int64_t l = 0; l < LP; ++l)
    if (h->dirty[(size_t)l]) h->col_streams.push_back((int32_t)l);
  if (h->col_streams.empty()) return AF_OK;
  const size_t n = h->col_streams.size();
  h->col64.resize(n * af::kLcF64Rows);
  h->col32.resize(n * af::kLcF32Fixed);
  for (size_t i = 0; i < n; ++i) {
    const int32_t l = h->col_streams[i];
    const bool set = l < h->n_streams && h->configured[(size_t)l];  // a padded lane runs the defaults on zeros
    lc_column(h, set ? &h->settings[(size_t)l] : nullptr, &h->col64[i * af::kLcF64Rows], &h->col32[i * af::kLcF32Fixed]);
  }
  AF_HIP(h->d_col64.reserve_exact(sizeof(double) * h->col64.size()));
  AF_HIP(h->d_col32.reserve_exact(sizeof(uint32_t) * h->col32.size()));
  AF_HIP(h->d_streams.reserve_exact(sizeof(int32_t) * n));
  // The host does not wait: the columns leave through pinned slots, and the device-side records are rewritten only behind
  // this scatter (the next flush is on the same stream, or lc_process has waited for this one; growing them frees, which waits).
  AF_HIP(h->slots.upload(h->d_col64, h->col64.data(), sizeof(double) * h->col64.size(), q));
  AF_HIP(h->slots.upload(h->d_col32, h->col32.data(), sizeof(uint32_t) * h->col32.size(), q));
  AF_HIP(h->slots.upload(h->d_streams, h->col_streams.data(), sizeof(int32_t) * n, q));
  af::LaneChainScatterArgs sc{};
  sc.col64 = h->d_col64;
  sc.col32 = h->d_col32;
  sc.streams = h->d_streams;
  sc.p64 = h->d_p64;
  sc.p32 = h->d_p32;
  sc.n = (int32_t)n;
  sc.lanes_padded = (int32_t)LP;
  sc.f32_rows = f32_rows;
  AF_HIP(af::launch_lane_chain_scatter(sc, q));
  std::fill(h->dirty.begin(), h->dirty.end(), 0);
  return AF_OK;
}

int lc_process(af_lane_chain *h, const float *in, float *out, bool on_device, int64_t n, int64_t stride, hipStream_t q) {
  if (!h || !in || !out) return fail(AF_ERR_INVALID_ARGUMENT, "%s is null", !h ? "handle" : (!in ? "in" : "out"));
  if (n < 0) return fail(AF_ERR_INVALID_ARGUMENT, "n_samples must not be negative");
  if (stride < n) return fail(AF_ERR_INVALID_ARGUMENT, "stride must cover n_samples");
  if (n == 0) return AF_OK;
  const int64_t blocks = (n + h->control_block - 1) / h->control_block;
  DeviceScope scope(h->device);
  AF_HIP(scope.status());
  h->touched_device = true;
  if (h->last_stream != q) AF_HIP(hipStreamSynchronize(h->last_stream));  // one call at a time owns the planes and the rows
  if (int rc = lc_flush(h, q)) return rc;
  const size_t f4 = sizeof(float);
  const int32_t B = h->n_streams;
  const float *d_in = in;
  float *d_out = out;
  int64_t d_stride = stride;
  if (sizeof(af::BlockStats) * (size_t)blocks * B > h->d_rows.bytes()) {
    AF_HIP(hipStreamSynchronize(q));  // nothing still writes the rows that are replaced
    AF_HIP(h->d_rows.reserve_exact(sizeof(af::BlockStats) * (size_t)blocks * B));
  }
  if (!on_device) {
    if (f4 * (size_t)B * n > h->d_in.bytes()) AF_HIP(hipStreamSynchronize(q));
    AF_HIP(h->d_in.reserve_exact(f4 * (size_t)B * n));
    AF_HIP(h->d_out.reserve_exact(f4 * (size_t)B * n));
    AF_HIP(hipMemcpy2DAsync(h->d_in, f4 * n, in, f4 * stride, f4 * n, B, hipMemcpyHostToDevice, q));
    d_in = h->d_in;
    d_out = h->d_out;
    d_stride = n;
  }
  af::LaneChainArgs a{};
  a.in = d_in;
  a.out = d_out;
  a.p64 = h->d_p64;
  a.p32 = h->d_p32;
  a.rows = h->d_rows;
  a.uniform = h->uniform;
  a.stride = d_stride;
  a.n_samples = n;
  a.samples_before = h->samples_total;
  a.n_lanes = B;
  a.lanes_padded = h->lanes_padded;
  a.control_block = h->control_block;
  a.lookahead_samples = h->lookahead_samples;
  a.ring_position = (int32_t)(h->samples_total % (h->lookahead_samples + 1));
  AF_HIP(h->span.begin(q));
  AF_HIP(af::launch_lane_chain(a, q));
  AF_HIP(h->span.end(q));
  h->samples_total += n;
  for (int64_t &v : h->processed) v += n;
  h->blocks = blocks;
  h->last_stream = q;
  if (!on_device) {
    AF_HIP(hipMemcpy2DAsync(out, f4 * stride, h->d_out, f4 * n, f4 * n, B, hipMemcpyDeviceToHost, q));
    AF_HIP(hipStreamSynchronize(q));
  }
  return AF_OK;
}

bool lc_settings_finite(const af_lane_chain_settings &s) {
  for (int i = 0; i < af::kNumBands; ++i)
    for (int v = 0; v < 3; ++v)
      if (!std::isfinite(s.bands[i][v])) return false;
  const double values[] = {s.compressor_threshold_db, s.compressor_ratio, s.compressor_attack_ms, s.compressor_release_ms,
                           s.compressor_makeup_gain_db, s.compressor_base_release_ms, s.limiter_ceiling_db, s.limiter_release_ms};
  for (double v : values)
    if (!std::isfinite(v)) return false;
  return true;
}

}  // namespace

extern "C" {

int af_lane_chain_default_settings(af_lane_chain_settings *out) {
  if (!out) return fail(AF_ERR_INVALID_ARGUMENT, "out is null");
  af_lane_chain_settings s{};
  for (int i = 0; i < af::kNumBands; ++i) {
    s.bands[i][0] = af::kDefaultFrequencies[i];
    s.bands[i][1] = 0.0;
    s.bands[i][2] = af::kDefaultQ;
  }
  s.compressor_threshold_db = -20.0; s.compressor_ratio = 4.0; s.compressor_attack_ms = 10.0; s.compressor_release_ms = 200.0;
  s.compressor_makeup_gain_db = 0.0; s.compressor_base_release_ms = 50.0;
  s.limiter_ceiling_db = -0.5; s.limiter_release_ms = 50.0;
  s.eq_enabled = 1; s.compressor_enabled = 1; s.limiter_enabled = 1;
  s.compressor_adaptive_release = 0; s.compressor_sidechain_highpass_enabled = 1; s.limiter_careful_output_enabled = 1;
  *out = s;
  return AF_OK;
}

int af_lane_chain_create(double sample_rate, int32_t n_streams, double limiter_lookahead_ms, int32_t device, af_lane_chain **out) {
  if (!out) return fail(AF_ERR_INVALID_ARGUMENT, "out is null");
  *out = nullptr;
  if (!std::isfinite(sample_rate) || sample_rate <= 0.0) return fail(AF_ERR_INVALID_ARGUMENT, "sample_rate must be positive and finite");
  if (n_streams <= 0) return fail(AF_ERR_INVALID_ARGUMENT, "n_streams must be positive");
  if (!std::isfinite(limiter_lookahead_ms) || limiter_lookahead_ms <= 0.0)
    return fail(AF_ERR_INVALID_ARGUMENT, "limiter_lookahead_ms must be positive and finite");
  if (device < 0) return fail(AF_ERR_INVALID_ARGUMENT, "device must be >= 0");
  af_lane_chain *h = new af_lane_chain();
  h->sample_rate = sample_rate;
  h->lookahead_ms = limiter_lookahead_ms;
  h->device = device;
  h->n_streams = n_streams;
  h->lanes_padded = (int32_t)(((int64_t)n_streams + af::kLanes - 1) / af::kLanes * af::kLanes);
  const af::ChainProto proto(sample_rate);
  h->control_block = proto.control_block;  // python_api.rs:512-514
  h->lookahead_samples = af::LimiterProto::samples_for(limiter_lookahead_ms, sample_rate);
  h->uniform = proto.compressor.params(h->control_block);  // what depends on the sample rate alone (the knee is new()'s 6 dB)
  af_lane_chain_settings defaults;
  af_lane_chain_default_settings(&defaults);
  h->settings.assign((size_t)n_streams, defaults);
  h->configured.assign((size_t)n_streams, 0);
  h->dirty.assign((size_t)h->lanes_padded, 1);
  h->processed.assign((size_t)n_streams, 0);
  *out = h;
  return AF_OK;
}

void af_lane_chain_destroy(af_lane_chain *h) { delete h; }

int af_lane_chain_configure(af_lane_chain *h, const int32_t *streams, int32_t n, const af_lane_chain_settings *settings) {
  if (!h) return fail(AF_ERR_INVALID_ARGUMENT, "handle is null");
  if (!streams) return fail(AF_ERR_INVALID_ARGUMENT, "streams is null");
  if (!settings) return fail(AF_ERR_INVALID_ARGUMENT, "settings is null");
  if (n <= 0) return fail(AF_ERR_INVALID_ARGUMENT, "n must be positive");
  std::vector<uint8_t> seen((size_t)h->n_streams, 0);
  for (int32_t i = 0; i < n; ++i) {
    const int32_t s = streams[i];
    if (s < 0 || s >= h->n_streams) return fail(AF_ERR_INVALID_ARGUMENT, "streams[%d] = %d is out of range (0..%d)", i, s, h->n_streams - 1);
    if (seen[(size_t)s]) return fail(AF_ERR_INVALID_ARGUMENT, "streams[%d] = %d is listed twice", i, s);
    seen[(size_t)s] = 1;
    if (!lc_settings_finite(settings[i])) return fail(AF_ERR_INVALID_ARGUMENT, "settings[%d] (stream %d): values must be finite", i, s);
  }
  for (int32_t i = 0; i < n; ++i) {
    const size_t s = (size_t)streams[i];
    h->settings[s] = settings[i];
    h->configured[s] = 1;
    h->dirty[s] = 1;
    h->processed[s] = 0;
  }
  return AF_OK;
}

int af_lane_chain_process_host(af_lane_chain *h, const float *in, float *out, int64_t n_samples, int64_t stride) {
  return lc_process(h, in, out, false, n_samples, stride, nullptr);
}

int af_lane_chain_process_device(af_lane_chain *h, const float *d_in, float *d_out, int64_t n_samples, int64_t stride, void *hip_stream) {
  return lc_process(h, d_in, d_out, true, n_samples, stride, static_cast<hipStream_t>(hip_stream));
}

int64_t af_lane_chain_blocks(const af_lane_chain *h) { return h ? h->blocks : 0; }

int af_lane_chain_read_rows(af_lane_chain *h, af_block_stats *rows, int64_t capacity) {
  if (!h) return fail(AF_ERR_INVALID_ARGUMENT, "handle is null");
  if (!rows) return fail(AF_ERR_INVALID_ARGUMENT, "rows is null");
  if (h->blocks == 0) return fail(AF_ERR_STATE, "no process call has been made");
  const size_t count = (size_t)h->blocks * h->n_streams;
  if (capacity < (int64_t)count) return fail(AF_ERR_INVALID_ARGUMENT, "rows must hold %zu records", count);
  DeviceScope scope(h->device);
  AF_HIP(scope.status());
  AF_HIP(hipStreamSynchronize(h->last_stream));
  AF_HIP(hipMemcpy(rows, h->d_rows, sizeof(af_block_stats) * count, hipMemcpyDeviceToHost));
  return AF_OK;
}

int af_lane_chain_reset(af_lane_chain *h) {
  if (!h) return fail(AF_ERR_INVALID_ARGUMENT, "handle is null");
  std::fill(h->dirty.begin(), h->dirty.end(), 1);
  std::fill(h->processed.begin(), h->processed.end(), 0);
  return AF_OK;
}

int af_lane_chain_samples_processed(const af_lane_chain *h, int32_t stream, int64_t *out) {
  if (!h) return fail(AF_ERR_INVALID_ARGUMENT, "handle is null");
  if (!out) return fail(AF_ERR_INVALID_ARGUMENT, "out is null");
  if (stream < 0 || stream >= h->n_streams) return fail(AF_ERR_INVALID_ARGUMENT, "stream %d is out of range (0..%d)", stream, h->n_streams - 1);
  *out = h->processed[(size_t)stream];
  return AF_OK;
}

int af_lane_chain_last_kernel_ms(af_lane_chain *h, double *ms) {
  if (!h) return fail(AF_ERR_INVALID_ARGUMENT, "handle is null");
  if (!ms) return fail(AF_ERR_INVALID_ARGUMENT, "ms is null");
  *ms = 0.0;
  if (!h->span.used()) return AF_OK;
  DeviceScope scope(h->device);
  AF_HIP(scope.status());
  AF_HIP(h->span.elapsed_ms(ms));
  return AF_OK;
}

}  // extern "C"
