// af_api_compressor_search.cpp -- the C ABI of the compressor candidate sweep (af_compressor_search_*): the simulations behind
// python/mic_eq/analysis/voice_setup.py:699-1079.  The kernels are af_compressor_search.hip's; the lanes' compressor parameters
// come from the host mirror of the reference's setters (af_host.hpp), what is per capture from af_compressor_search_math.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "af_api_internal.hpp"
#include "af_compressor_search_host.hpp"
#include "af_compressor_search_math.h"
#include "af_host.hpp"

struct af_compressor_search {
  int device = 0;
  double sample_rate = 48000.0;
  bool touched_device = false;
  int control_block = 960;
  af::LimiterProto limiter;
  af::TruePeakProto tp;
  float effective_ceiling_db = -1.5f;
  // the loaded batch
  int32_t n_captures = 0, n_blocks = 0;
  int64_t n_samples = 0, stride = 0;
  const float *d_in = nullptr;  // d_audio, or the caller's device pointer
  std::vector<af_block_stats> input_rows;  // [blocks][captures]
  std::vector<float> in_db, active_threshold_db;  // [captures][blocks], [captures]
  std::vector<uint8_t> mask;                      // [captures][blocks]
  af::DeviceBuffer<float> d_audio, d_in_db, d_dees, d_ring, d_out_audio;
  af::DeviceBuffer<uint8_t> d_mask;
  af::DeviceBuffer<af::CsCapture> d_captures;
  // the last sweep
  int32_t n_lanes = 0;
  bool kept_audio = false;
  std::vector<int32_t> lane_capture;
  af::DeviceBuffer<double> d_lane_f64;
  af::DeviceBuffer<int32_t> d_lane_capture;
  af::DeviceBuffer<uint32_t> d_lane_flags;
  af::DeviceBuffer<af::CsRow> d_rows;
  af::DeviceBuffer<af_chain_simulation> d_results;
  af::TimedSpan sweep_span, fold_span;
  double run_ms[6] = {};  // the last run's three sweeps: sweep and fold kernel each

  explicit af_compressor_search(double fs) : sample_rate(fs), limiter(-0.5, 50.0, fs, 2.0), tp((float)fs, -1.5f, 80.0f) {}
  ~af_compressor_search() {
    if (touched_device) { (void)hipSetDevice(device); (void)hipDeviceSynchronize(); }
  }
};

namespace {

int cs_set_limiter(af_compressor_search *h, double ceiling_db, double release_ms, double lookahead_ms, bool careful) {
  // python_api.rs:472-487; effective_limiter_ceiling_db, control.rs:904-910, then `as f32`
  const float effective = (float)(careful ? std::fmin(ceiling_db, -1.5) : ceiling_db);
  h->limiter.set_lookahead_ms(lookahead_ms);
  h->limiter.set_ceiling((double)effective);
  h->limiter.set_release_time(release_ms);
  h->tp.set_release_ms((float)release_ms);
  h->effective_ceiling_db = effective;
  return AF_OK;
}

bool all_finite(const double *v, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

// what evaluate() reads of a simulation (voice_setup.py:824-847); Python's float() of an f32 is the widened value
csm_simulation to_csm(const af_chain_simulation &r) {
  csm_simulation s{};
  s.peak = r.compressor_gain_reduction_db;
  s.median = r.compressor_gain_reduction_median_db;
  s.p95 = r.compressor_gain_reduction_p95_db;
  s.active_ratio = r.compressor_gain_reduction_active_ratio;
  s.active_gain = r.active_output_gain_db;
  s.output_true_peak = r.output_true_peak_db;
  s.ceiling = r.limiter_effective_ceiling_db;
  s.pre_limiter_headroom = r.pre_limiter_true_peak_headroom_db;
  s.pumping = r.compressor_pumping_score_db;
  s.silence_gain = r.silence_output_gain_db;
  s.non_finite = r.non_finite_output != 0;
  return s;
}

int cs_load(af_compressor_search *h, const float *audio, bool on_device, int64_t n, int32_t C, int64_t stride, const af_block_stats *rows) {
  if (!h || !audio || !rows) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  if (C <= 0) return fail(AF_ERR_INVALID_ARGUMENT, "n_captures must be positive");
  if (n <= 0) return fail(AF_ERR_INVALID_ARGUMENT, "n_samples must be positive");
  if (stride < n) return fail(AF_ERR_INVALID_ARGUMENT, "stride must cover n_samples");
  const int64_t blocks = (n + h->control_block - 1) / h->control_block;
  if (blocks > af::kCsMaxBlocks)
    return fail(AF_ERR_UNSUPPORTED, "%lld control blocks per capture: the fold holds at most %d (%.2f s)", (long long)blocks, af::kCsMaxBlocks,
                af::kCsMaxBlocks * h->control_block / h->sample_rate);
  if (!on_device && !af::check_finite(audio, C, n, stride)) return fail(AF_ERR_NON_FINITE, "audio must contain only finite samples");
  AF_HIP(hipSetDevice(h->device));
  h->touched_device = true;
  AF_HIP(hipDeviceSynchronize());  // nothing of an earlier sweep still reads what is replaced
  h->n_captures = 0;
  const int nb = (int)blocks;
  std::vector<float> in_db((size_t)C * nb), dees((size_t)C * nb), scratch((size_t)nb);
  std::vector<uint8_t> mask((size_t)C * nb);
  std::vector<af::CsCapture> caps((size_t)C);
  for (int c = 0; c < C; ++c) {
    af::CsCapture &k = caps[(size_t)c];
    k = af::CsCapture{};
    k.active_count = csm_capture_masks(&rows[c].input_square_sum, (int64_t)C * (int64_t)(sizeof(af_block_stats) / sizeof(double)), nb, n,
                                       h->control_block, &in_db[(size_t)c * nb], &mask[(size_t)c * nb], scratch.data(),
                                       &k.active_threshold_db);
    double total = 0.0;  // the accumulation order of python_api.rs:519-571
    for (int i = 0; i < nb; ++i) {
      const af_block_stats &r = rows[(size_t)i * C + c];
      total += r.input_square_sum;
      k.input_sample_peak = std::fmax(k.input_sample_peak, r.input_sample_peak);
      k.deesser_max_db = std::fmax(k.deesser_max_db, r.deesser_gain_reduction_db);
      dees[(size_t)c * nb + i] = r.deesser_gain_reduction_db;
    }
    k.input_rms = (float)std::sqrt(total / (double)n);
  }
  const size_t f4 = sizeof(float);
  if (on_device) {
    h->d_in = audio;
    h->stride = stride;
  } else {
    AF_HIP(h->d_audio.reserve_exact(f4 * (size_t)C * n));
    AF_HIP(hipMemcpy2D(h->d_audio, f4 * n, audio, f4 * stride, f4 * n, C, hipMemcpyHostToDevice));
    h->d_in = h->d_audio;
    h->stride = n;
  }
  AF_HIP(h->d_in_db.reserve_exact(f4 * in_db.size()));
  AF_HIP(h->d_dees.reserve_exact(f4 * dees.size()));
  AF_HIP(h->d_mask.reserve_exact(mask.size()));
  AF_HIP(h->d_captures.reserve_exact(sizeof(af::CsCapture) * caps.size()));
  AF_HIP(hipMemcpy(h->d_in_db, in_db.data(), f4 * in_db.size(), hipMemcpyHostToDevice));
  AF_HIP(hipMemcpy(h->d_dees, dees.data(), f4 * dees.size(), hipMemcpyHostToDevice));
  AF_HIP(hipMemcpy(h->d_mask, mask.data(), mask.size(), hipMemcpyHostToDevice));
  AF_HIP(hipMemcpy(h->d_captures, caps.data(), sizeof(af::CsCapture) * caps.size(), hipMemcpyHostToDevice));
  h->input_rows.assign(rows, rows + (size_t)nb * C);
  h->active_threshold_db.resize((size_t)C);
  for (int c = 0; c < C; ++c) h->active_threshold_db[(size_t)c] = caps[(size_t)c].active_threshold_db;
  h->in_db = std::move(in_db);
  h->mask = std::move(mask);
  h->n_samples = n;
  h->n_blocks = nb;
  h->n_lanes = 0;
  h->kept_audio = false;
  h->n_captures = C;
  return AF_OK;
}

}  // namespace

extern "C" {

int af_compressor_search_create(double sample_rate, int32_t device, af_compressor_search **out) {
  if (!out) return fail(AF_ERR_INVALID_ARGUMENT, "out is null");
  *out = nullptr;
  if (!std::isfinite(sample_rate) || sample_rate <= 0.0) return fail(AF_ERR_INVALID_ARGUMENT, "sample_rate must be positive and finite");
  if (device < 0) return fail(AF_ERR_INVALID_ARGUMENT, "device must be >= 0");
  af_compressor_search *h = new af_compressor_search(sample_rate);
  h->device = device;
  h->control_block = (int)std::min(8192.0, std::max(1.0, std::round(sample_rate * 0.020)));  // python_api.rs:512-514
  cs_set_limiter(h, -1.5, 80.0, 2.0, true);  // voice_setup.py:748-753
  *out = h;
  return AF_OK;
}

void af_compressor_search_destroy(af_compressor_search *h) { delete h; }

int af_compressor_search_set_limiter(af_compressor_search *h, double ceiling_db, double release_ms, double lookahead_ms,
                                     int32_t careful_output) {
  if (!h) return fail(AF_ERR_INVALID_ARGUMENT, "handle is null");
  if (!std::isfinite(ceiling_db) || !std::isfinite(release_ms) || !std::isfinite(lookahead_ms))
    return fail(AF_ERR_INVALID_ARGUMENT, "limiter settings must be finite");
  return cs_set_limiter(h, ceiling_db, release_ms, lookahead_ms, careful_output != 0);
}

int af_compressor_search_load_host(af_compressor_search *h, const float *audio, int64_t n_samples, int32_t n_captures, int64_t stride,
                                   const af_block_stats *input_rows) {
  return cs_load(h, audio, false, n_samples, n_captures, stride, input_rows);
}

int af_compressor_search_load_device(af_compressor_search *h, const float *d_audio, int64_t n_samples, int32_t n_captures,
                                     int64_t stride, const af_block_stats *input_rows) {
  return cs_load(h, d_audio, true, n_samples, n_captures, stride, input_rows);
}

int64_t af_compressor_search_blocks(const af_compressor_search *h) { return h && h->n_captures ? h->n_blocks : 0; }

int af_compressor_search_read_masks(const af_compressor_search *h, float *in_db, uint8_t *mask, float *active_threshold_db) {
  if (!h) return fail(AF_ERR_INVALID_ARGUMENT, "handle is null");
  if (h->n_captures == 0) return fail(AF_ERR_STATE, "no captures are loaded");
  if (in_db) std::copy(h->in_db.begin(), h->in_db.end(), in_db);
  if (mask) std::copy(h->mask.begin(), h->mask.end(), mask);
  if (active_threshold_db) std::copy(h->active_threshold_db.begin(), h->active_threshold_db.end(), active_threshold_db);
  return AF_OK;
}

int af_compressor_search_sweep(af_compressor_search *h, const af_compressor_candidate *lanes, int32_t n_lanes,
                               const af_compressor_base *bases, int32_t keep_audio, af_chain_simulation *out) {
  if (!h || !lanes || !bases || !out) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  if (h->n_captures == 0) return fail(AF_ERR_STATE, "no captures are loaded");
  if (n_lanes <= 0) return fail(AF_ERR_INVALID_ARGUMENT, "n_lanes must be positive");
  for (int32_t l = 0; l < n_lanes; ++l) {
    const af_compressor_candidate &c = lanes[l];
    if (c.capture < 0 || c.capture >= h->n_captures)
      return fail(AF_ERR_INVALID_ARGUMENT, "lane %d names capture %d of %d", l, c.capture, h->n_captures);
    if (!std::isfinite(c.threshold_db) || !std::isfinite(c.ratio) || !std::isfinite(c.attack_ms) || !std::isfinite(c.release_ms))
      return fail(AF_ERR_INVALID_ARGUMENT, "lane %d: candidate values must be finite", l);
  }
  for (int32_t c = 0; c < h->n_captures; ++c)
    if (!std::isfinite(bases[c].makeup_gain_db) || !std::isfinite(bases[c].base_release_ms))
      return fail(AF_ERR_INVALID_ARGUMENT, "capture %d: base settings must be finite", c);
  AF_HIP(hipSetDevice(h->device));
  const int64_t LP = ((int64_t)n_lanes + af::kLanes - 1) / af::kLanes * af::kLanes;
  const int W = h->limiter.lookahead_samples + 1;
  const int nb = h->n_blocks;

  // every lane's compressor: Compressor::new (block_processor.rs:46-60) and the setters in python_api.rs:446-470's order
  std::vector<double> f64((size_t)af::kCsLaneFields * LP);
  std::vector<uint32_t> flags((size_t)LP);
  h->lane_capture.assign((size_t)LP, 0);
  af::CompressorParams uniform{};
  for (int64_t l = 0; l < LP; ++l) {
    const af_compressor_candidate &c = lanes[std::min<int64_t>(l, n_lanes - 1)];  // the padding repeats the last lane
    const af_compressor_base &b = bases[c.capture];
    af::CompressorProto p(-18.0, 3.0, 5.0, 100.0, 0.0, 6.0, h->sample_rate);
    p.set_threshold(c.threshold_db);
    p.set_ratio(c.ratio);
    p.set_attack_time(c.attack_ms);
    p.set_release_time(c.release_ms);
    p.set_makeup_gain(b.makeup_gain_db);
    p.set_adaptive_release(b.adaptive_release != 0);
    p.set_base_release_time(b.base_release_ms);
    p.set_auto_makeup_enabled(false);
    p.set_sidechain_highpass_enabled(b.sidechain_highpass_enabled != 0);
    const af::CompressorParams q = p.params(h->control_block);
    if (l == 0) uniform = q;
    double *f = &f64[(size_t)l];
    f[(size_t)af::kCsThresholdDb * LP] = q.threshold_db;
    f[(size_t)af::kCsAttackCoeff * LP] = q.attack_coeff;
    f[(size_t)af::kCsDetectorReleaseCoeff * LP] = q.detector_release_coeff;
    f[(size_t)af::kCsBaseReleaseMs * LP] = q.base_release_ms;
    f[(size_t)af::kCsMakeupGainDb * LP] = q.makeup_gain_db;
    f[(size_t)af::kCsCompFactor * LP] = q.comp_factor;
    f[(size_t)af::kCsKneeStart * LP] = q.knee_start;
    f[(size_t)af::kCsKneeEnd * LP] = q.knee_end;
    f[(size_t)af::kCsCurReleaseMs * LP] = p.current_release_ms;
    f[(size_t)af::kCsTargetReleaseMs * LP] = p.target_release_ms;
    f[(size_t)af::kCsReleaseCoeff * LP] = af::time_constant_to_coeff(p.current_release_ms, p.sample_rate);  // compressor.rs:760-761
    f[(size_t)af::kCsSmoothedMakeup * LP] = p.smoothed_makeup_gain;
    flags[(size_t)l] = (q.adaptive_release ? af::kCsAdaptiveRelease : 0u) | (q.sidechain_highpass_enabled ? af::kCsSidechainHighpass : 0u);
    h->lane_capture[(size_t)l] = c.capture;
  }

  AF_HIP(hipDeviceSynchronize());
  h->n_lanes = 0;
  h->kept_audio = false;
  const size_t ring_bytes = sizeof(float) * 2 * (size_t)W * LP;
  AF_HIP(h->d_lane_f64.reserve_exact(sizeof(double) * f64.size()));
  AF_HIP(h->d_lane_capture.reserve_exact(sizeof(int32_t) * (size_t)LP));
  AF_HIP(h->d_lane_flags.reserve_exact(sizeof(uint32_t) * (size_t)LP));
  AF_HIP(h->d_ring.reserve_exact(ring_bytes));
  AF_HIP(h->d_rows.reserve_exact(sizeof(af::CsRow) * (size_t)nb * n_lanes));
  AF_HIP(h->d_results.reserve_exact(sizeof(af_chain_simulation) * (size_t)n_lanes));
  if (keep_audio) AF_HIP(h->d_out_audio.reserve_exact(sizeof(float) * (size_t)n_lanes * h->n_samples));
  AF_HIP(hipMemcpy(h->d_lane_f64, f64.data(), sizeof(double) * f64.size(), hipMemcpyHostToDevice));
  AF_HIP(hipMemcpy(h->d_lane_capture, h->lane_capture.data(), sizeof(int32_t) * (size_t)LP, hipMemcpyHostToDevice));
  AF_HIP(hipMemcpy(h->d_lane_flags, flags.data(), sizeof(uint32_t) * (size_t)LP, hipMemcpyHostToDevice));
  hipStream_t q = nullptr;
  AF_HIP(hipMemsetAsync(h->d_ring, 0, ring_bytes, q));

  af::CsSweepArgs sw{};
  sw.in = h->d_in;
  sw.lane_f64 = h->d_lane_f64;
  sw.lane_capture = h->d_lane_capture;
  sw.lane_flags = h->d_lane_flags;
  sw.ring = h->d_ring;
  sw.rows = h->d_rows;
  sw.audio = keep_audio ? h->d_out_audio.get() : nullptr;
  sw.uniform = uniform;
  sw.lim = h->limiter.params();
  // block_processor.rs:150-151: the TP ceiling follows the limiter ceiling on every block
  af::TruePeakProto tp = h->tp;
  tp.set_ceiling_linear(std::pow(10.0f, (float)h->limiter.ceiling_db / 20.0f));
  sw.tp.ceiling_linear = tp.ceiling_linear;
  sw.tp.release_coeff = tp.release_coeff;
  sw.stride = h->stride;
  sw.n_samples = h->n_samples;
  sw.n_lanes = n_lanes;
  sw.lanes_padded = (int32_t)LP;
  sw.control_block = h->control_block;
  AF_HIP(h->sweep_span.begin(q));
  AF_HIP(af::launch_cs_sweep(sw, q));
  AF_HIP(h->sweep_span.end(q));

  af::CsFoldArgs fo{};
  fo.rows = h->d_rows;
  fo.lane_capture = h->d_lane_capture;
  fo.in_db = h->d_in_db;
  fo.deesser_db = h->d_dees;
  fo.mask = h->d_mask;
  fo.captures = h->d_captures;
  fo.out = h->d_results;
  fo.n_samples = h->n_samples;
  fo.n_lanes = n_lanes;
  fo.n_blocks = nb;
  fo.control_block = h->control_block;
  fo.ceiling_db = h->effective_ceiling_db;
  csm_pumping_alphas(50.0f, &fo.highpass_alpha, &fo.lowpass_alpha);
  AF_HIP(h->fold_span.begin(q));
  AF_HIP(af::launch_cs_fold(fo, q));
  AF_HIP(h->fold_span.end(q));
  AF_HIP(hipMemcpy(out, h->d_results, sizeof(af_chain_simulation) * (size_t)n_lanes, hipMemcpyDeviceToHost));
  h->n_lanes = n_lanes;
  h->kept_audio = keep_audio != 0;
  return AF_OK;
}

int af_compressor_search_run(af_compressor_search *h, const af_compressor_search_settings *settings, af_compressor_search_result *out) {
  if (!h || !settings || !out) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  if (h->n_captures == 0) return fail(AF_ERR_STATE, "no captures are loaded");
  const int C = h->n_captures;
  std::vector<csm_search> searches((size_t)C);
  std::vector<af_compressor_base> bases((size_t)C);
  for (int c = 0; c < C; ++c) {
    const af_compressor_search_settings &s = settings[c];
    const double values[] = {s.threshold_db, s.ratio, s.attack_ms, s.release_ms, s.makeup_gain_db, s.base_release_ms, s.target_lufs,
                             s.measured_short_term_lufs, s.target_p95_db, s.target_median_db, s.peak_cap_db};
    if (!all_finite(values, sizeof values / sizeof values[0])) return fail(AF_ERR_INVALID_ARGUMENT, "capture %d: settings must be finite", c);
    csm_settings cs{};
    cs.compressor[0] = s.threshold_db; cs.compressor[1] = s.ratio; cs.compressor[2] = s.attack_ms; cs.compressor[3] = s.release_ms;
    cs.auto_makeup_enabled = s.auto_makeup_enabled != 0;
    cs.target_lufs = s.target_lufs;
    cs.measured_short_term_lufs = s.measured_short_term_lufs;
    cs.target_p95_db = s.target_p95_db; cs.target_median_db = s.target_median_db; cs.peak_cap_db = s.peak_cap_db;
    csm_begin(&searches[(size_t)c], &cs);
    // voice_setup.py:798-801: the simulated compressor has auto-makeup off, and makeup 0 when the settings have it on
    bases[(size_t)c] = af_compressor_base{s.auto_makeup_enabled ? 0.0 : s.makeup_gain_db, s.base_release_ms, s.adaptive_release,
                                          s.sidechain_highpass_enabled};
  }
  // every capture's simulation records, in evaluation order
  std::vector<std::vector<af_chain_simulation>> records((size_t)C);
  std::vector<af_compressor_candidate> lanes;
  std::vector<af_chain_simulation> results;
  std::fill(h->run_ms, h->run_ms + 6, 0.0);
  int phase = 0;
  const auto simulate_waiting = [&]() -> int {  // entries[n_scored .. n) of every search: one sweep, scored in order
    lanes.clear();
    for (int c = 0; c < C; ++c) {
      const csm_search &s = searches[(size_t)c];
      for (int i = s.n_scored; i < s.n; ++i)
        lanes.push_back(af_compressor_candidate{c, 0, s.entries[i].values[0], s.entries[i].values[1], s.entries[i].values[2], s.entries[i].values[3]});
    }
    if (lanes.empty()) return AF_OK;
    results.resize(lanes.size());
    if (int rc = af_compressor_search_sweep(h, lanes.data(), (int32_t)lanes.size(), bases.data(), 0, results.data())) return rc;
    if (int rc = af_compressor_search_last_kernel_ms(h, &h->run_ms[2 * phase], &h->run_ms[2 * phase + 1])) return rc;
    size_t l = 0;
    for (int c = 0; c < C; ++c) {
      csm_search &s = searches[(size_t)c];
      while (s.n_scored < s.n) {
        const csm_simulation sim = to_csm(results[l]);
        records[(size_t)c].push_back(results[l++]);
        csm_score(&s, &sim);
      }
    }
    return AF_OK;
  };
  for (int c = 0; c < C; ++c) csm_phase1(&searches[(size_t)c]);
  if (int rc = simulate_waiting()) return rc;
  phase = 1;
  for (int c = 0; c < C; ++c) (void)csm_phase2(&searches[(size_t)c]);  // (no feasible candidate: nothing is listed)
  if (int rc = simulate_waiting()) return rc;

  // the choice, then the winners' verification runs
  std::vector<csm_choice> choices((size_t)C);
  lanes.clear();
  for (int c = 0; c < C; ++c) {
    csm_choose(&searches[(size_t)c], &choices[(size_t)c]);
    if (!choices[(size_t)c].feasible) continue;
    const double *v = searches[(size_t)c].entries[choices[(size_t)c].best].values;
    lanes.push_back(af_compressor_candidate{c, 0, v[0], v[1], v[2], v[3]});
  }
  results.resize(lanes.size());
  if (!lanes.empty()) {
    if (int rc = af_compressor_search_sweep(h, lanes.data(), (int32_t)lanes.size(), bases.data(), 0, results.data())) return rc;
    if (int rc = af_compressor_search_last_kernel_ms(h, &h->run_ms[4], &h->run_ms[5])) return rc;
  }
  size_t l = 0;
  for (int c = 0; c < C; ++c) {
    const csm_search &s = searches[(size_t)c];
    const csm_choice &ch = choices[(size_t)c];
    af_compressor_search_result &r = out[c];
    r = af_compressor_search_result{};
    r.evaluated_count = s.n_scored;
    for (int i = 0; i < s.n_scored; ++i) {
      std::copy(s.entries[i].values, s.entries[i].values + CSM_CONTROLS, r.evaluated[i]);
      r.scores[i] = s.entries[i].score;
    }
    r.winner = -1;
    r.threshold_db = settings[c].threshold_db; r.ratio = settings[c].ratio;
    r.attack_ms = settings[c].attack_ms; r.release_ms = settings[c].release_ms;
    r.incumbent_objective = ch.incumbent_objective;
    r.threshold_only_objective = ch.threshold_only_objective;
    if (!ch.feasible) {
      r.iterations = s.n_scored;  // :933
      continue;
    }
    const af_chain_simulation &sim = results[l++];
    const csm_entry &best = s.entries[ch.best];
    r.backend_available = 1;
    r.winner = ch.best;
    r.verification_equals_evaluation = std::memcmp(&sim, &records[(size_t)c][(size_t)ch.best], sizeof sim) == 0;
    r.threshold_db = best.values[0]; r.ratio = best.values[1]; r.attack_ms = best.values[2]; r.release_ms = best.values[3];
    r.expanded_search_selected = ch.expanded_selected;
    r.measured_median_gain_reduction_db = sim.compressor_gain_reduction_median_db;
    r.measured_p95_gain_reduction_db = sim.compressor_gain_reduction_p95_db;
    r.measured_peak_gain_reduction_db = sim.compressor_gain_reduction_db;
    r.active_reduction_ratio = sim.compressor_gain_reduction_active_ratio;
    r.peak_cap_passed = (double)sim.compressor_gain_reduction_db <= settings[c].peak_cap_db + 1.0e-6;
    r.total_objective = best.score;
    r.expanded_candidate_objective = s.entries[ch.expanded].score;
    r.active_output_gain_db = sim.active_output_gain_db;
    r.silence_output_gain_db = sim.silence_output_gain_db;
    r.compressor_pumping_score_db = sim.compressor_pumping_score_db;
    r.output_true_peak_db = sim.output_true_peak_db;
    r.pre_limiter_true_peak_headroom_db = sim.pre_limiter_true_peak_headroom_db;
    r.candidate_count = r.iterations = s.n_scored + 1;  // :1068-1069
  }
  return AF_OK;
}

int af_compressor_search_last_run_ms(const af_compressor_search *h, double ms[6]) {
  if (!h || !ms) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  std::copy(h->run_ms, h->run_ms + 6, ms);
  return AF_OK;
}

int af_compressor_search_read_rows(af_compressor_search *h, af_block_stats *rows, int64_t capacity) {
  if (!h || !rows) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  if (h->n_lanes == 0) return fail(AF_ERR_STATE, "no sweep has run on the loaded captures");
  const size_t count = (size_t)h->n_blocks * h->n_lanes;
  if (capacity < (int64_t)count) return fail(AF_ERR_INVALID_ARGUMENT, "rows must hold %zu records", count);
  AF_HIP(hipSetDevice(h->device));
  std::vector<af::CsRow> lane_rows(count);
  AF_HIP(hipMemcpy(lane_rows.data(), h->d_rows, sizeof(af::CsRow) * count, hipMemcpyDeviceToHost));
  for (int i = 0; i < h->n_blocks; ++i)
    for (int l = 0; l < h->n_lanes; ++l) {
      const af::CsRow &r = lane_rows[(size_t)i * h->n_lanes + l];
      const af_block_stats &shared = h->input_rows[(size_t)i * h->n_captures + h->lane_capture[(size_t)l]];
      af_block_stats &o = rows[(size_t)i * h->n_lanes + l];
      o = af_block_stats{};
      o.input_sample_peak = shared.input_sample_peak;
      o.input_square_sum = shared.input_square_sum;
      o.deesser_gain_reduction_db = shared.deesser_gain_reduction_db;
      o.output_sample_peak = r.output_sample_peak;
      o.true_peak_limiter_input_peak = r.tp_limiter_input_peak;
      o.output_true_peak = r.output_true_peak;
      o.limiter_peak_gain_reduction_db = r.limiter_peak_gr_db;
      o.true_peak_limiter_gain_reduction_db = r.tp_limiter_gr_db;
      o.compressor_gain_reduction_db = r.compressor_gr_db;
      o.output_square_sum = r.output_square_sum;
      o.true_peak_limited_events = r.tp_limited_events;
      o.non_finite_output = r.non_finite_output;
      o.compressor_makeup_gain_db = r.makeup_gain_db;
    }
  return AF_OK;
}

int af_compressor_search_read_audio(af_compressor_search *h, float *audio, int64_t stride) {
  if (!h || !audio) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  if (h->n_lanes == 0 || !h->kept_audio) return fail(AF_ERR_STATE, "the last sweep kept no output audio");
  if (stride < h->n_samples) return fail(AF_ERR_INVALID_ARGUMENT, "stride must cover n_samples");
  AF_HIP(hipSetDevice(h->device));
  const size_t f4 = sizeof(float);
  AF_HIP(hipMemcpy2D(audio, f4 * stride, h->d_out_audio, f4 * h->n_samples, f4 * h->n_samples, h->n_lanes, hipMemcpyDeviceToHost));
  return AF_OK;
}

int af_compressor_search_last_kernel_ms(af_compressor_search *h, double *sweep_ms, double *fold_ms) {
  if (!h || !sweep_ms || !fold_ms) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  *sweep_ms = *fold_ms = 0.0;
  if (!h->sweep_span.used() && !h->fold_span.used()) return AF_OK;
  AF_HIP(hipSetDevice(h->device));
  AF_HIP(h->sweep_span.elapsed_ms(sweep_ms));
  AF_HIP(h->fold_span.elapsed_ms(fold_ms));
  return AF_OK;
}

}  // extern "C"
