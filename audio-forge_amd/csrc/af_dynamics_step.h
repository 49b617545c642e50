// af_dynamics_step.h -- the per-sample dynamics step of a lane that carries its OWN compressor parameters: compressor
// sample, lookahead-limiter step, 4x true-peak limiter step, output observation, and the block-end makeup smoothing.  One copy
// for the kernels that run it per lane: the candidate sweep (af_compressor_search.hip) and the streaming lane chain
// (af_lane_chain.hip).  The operations and their order are chain_lane_kernel's (af_kernels.hip), which keeps its own copy so
// that its code object is untouched.
//
// Memory the steps use: the two 32-tap true-peak histories are 32-row rings `float ring[kTpTaps][kLanes]` (LDS), addressed by
// the low five bits of a sample index `t`; the limiter's delay ring and suffix maxima are lane-major rows in global memory
// (row r of a lane at ring[r * LP], LP = padded lane count), addressed by the position `j` in the van-Herk block of W inputs.
#pragma once
#include <hip/hip_runtime.h>

#include "af_dsp.h"

namespace af {

struct DynCompState {
  double sc_prev_in, sc_prev_out, low_env, voiced_env, presence_env, plosive;
  double peak_env_db, rms_env_sq, gr, fast_env, slow_env, cur_release_ms, target_release_ms;
  double release_coeff, smoothed_makeup;
};

// Compressor::process_sample_impl(update_makeup_gain = false), dsp/compressor.rs:725-774 -- af_kernels.hip's comp_sample
__device__ __forceinline__ float dyn_comp_sample(const CompressorParams &p, DynCompState &s, float input, double makeup_lin) {
  const double x = (double)input;
  double d = x;
  double weight_db = kDetectorUnitWeight;
  if (p.sidechain_highpass_enabled) {
    // process_sidechain_sample, compressor.rs:407-417
    d = p.sidechain_highpass_coeff * (s.sc_prev_out + x - s.sc_prev_in);
    s.sc_prev_in = x;
    s.sc_prev_out = d;
    // update_sidechain_band_metrics, compressor.rs:420-450
    const double low = x - d;
    const double voiced = d;
    const double presence = 0.65 * d + 0.35 * (d - low);
    const double k = p.band_env_coeff;
    s.low_env = k * s.low_env + (1.0 - k) * low * low;
    s.voiced_env = k * s.voiced_env + (1.0 - k) * voiced * voiced;
    s.presence_env = k * s.presence_env + (1.0 - k) * presence * presence;
    const double low_rms = sqrt(s.low_env);
    const double voiced_rms = fmax(sqrt(s.voiced_env), 1e-8);
    const double presence_rms = sqrt(s.presence_env);
    s.plosive = dclamp(low_rms / voiced_rms, 0.0, 32.0);
    const double plosive_amount = dclamp(div_known(s.plosive - 1.25, 3.75, 1.0 / 3.75), 0.0, 1.0);
    const double plosive_penalty = 1.0 - plosive_amount * (1.0 - 0.35);
    const double presence_ratio = dclamp(presence_rms / voiced_rms, 0.0, 4.0);
    const double presence_weight = 1.0 + 0.18 * dclamp(presence_ratio - 0.75, 0.0, 1.0);
    const double w = dclamp(plosive_penalty * presence_weight, 0.35, 1.15);
    weight_db = detector_weight(w);
  } else {
    s.plosive = 0.0;
  }
  const double inst_peak_db = lin2db(fabs(d), 1e-10);
  const double pk = inst_peak_db > s.peak_env_db ? p.attack_coeff : p.detector_release_coeff;
  s.peak_env_db = pk * s.peak_env_db + (1.0 - pk) * inst_peak_db;

  const double sq = d * d;
  s.rms_env_sq = p.rms_coeff * s.rms_env_sq + (1.0 - p.rms_coeff) * sq;
  const double rms_db = detector_rms_level(s.rms_env_sq);

  const double detector_db = af::detector_db(s.peak_env_db, rms_db, weight_db);  // blended_detector_db, compressor.rs:681-686

  // update_adaptive_release_time_meter + release smoothing, compressor.rs:452-466,752-761 (see af_kernels.hip on release_coeff)
  if (p.adaptive_release) {
    const double sustained = dclamp(div_known(s.slow_env, 6.0, 1.0 / 6.0), 0.0, 1.0);
    const double transient_bias = dclamp(div_known(s.fast_env - s.slow_env, 7.0, 1.0 / 7.0), 0.0, 1.0);
    const double syllabic = dclamp(sustained * sustained * (1.0 - 0.35 * transient_bias), 0.0, 1.0);
    s.target_release_ms = 50.0 + syllabic * (400.0 - 50.0);
  } else {
    s.target_release_ms = p.base_release_ms;
  }
  const double release_diff = s.target_release_ms - s.cur_release_ms;
  if (fabs(release_diff) > 1.0) {
    s.cur_release_ms = p.release_smoothing_coeff * s.cur_release_ms + (1.0 - p.release_smoothing_coeff) * s.target_release_ms;
  } else {
    s.cur_release_ms = s.target_release_ms;
  }

  const double target = comp_gain_reduction(p, detector_db);
  // smooth_gain_reduction, compressor.rs:468-505
  if (!p.adaptive_release) {
    const double k = target > s.gr ? p.attack_coeff : s.release_coeff;
    s.gr = k * s.gr + (1.0 - k) * target;
    s.fast_env = s.gr;
    s.slow_env = 0.0;
  } else {
    if (target > s.gr) {
      s.fast_env = p.attack_coeff * s.gr + (1.0 - p.attack_coeff) * target;
    } else {
      s.fast_env = p.fast_release_coeff * s.fast_env + (1.0 - p.fast_release_coeff) * target;
    }
    if (target > 3.0) {
      s.slow_env = p.slow_charge_coeff * s.slow_env + (1.0 - p.slow_charge_coeff) * target;
    } else {
      s.slow_env *= p.slow_release_coeff;
    }
    s.gr = fmax(s.fast_env, s.slow_env);
  }
  const double output_gain = db2lin(-s.gr) * makeup_lin;
  return (float)(x * output_gain);
}

// end of a control block: update_auto_makeup_gain with auto-makeup off (compressor.rs:604-617)
__device__ __forceinline__ void dyn_block_end_makeup(const CompressorParams &p, DynCompState &s, int blk_len) {
  const double makeup_coeff = pow(p.makeup_smoothing_coeff, (double)(blk_len < 1 ? 1 : blk_len));
  const double makeup_target = p.makeup_gain_db;
  const double diff = makeup_target - s.smoothed_makeup;
  if (fabs(diff) > 0.1) {
    s.smoothed_makeup = makeup_coeff * s.smoothed_makeup + (1.0 - makeup_coeff) * makeup_target;
  } else {
    s.smoothed_makeup = makeup_target;
  }
}

// Bandlimited4xPeak::observe, dsp/true_peak.rs:173-186, over a 32-row ring: h[k] = sample t-k lives at row (t - k) & 31
__device__ __forceinline__ float dyn_tp_observe(const float (*ring)[kLanes], int t, int lane) {
  float h[kTpTaps];
#pragma unroll
  for (int k = 0; k < kTpTaps; ++k) h[k] = ring[(t - k) & (kTpTaps - 1)][lane];
  float peak = fabsf(h[0]);
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < kTpTaps; ++k) acc = __builtin_fmaf(AF_TP_FIR[p][k], h[k], acc);
    peak = fmaxf(peak, fabsf(acc));
  }
  return peak;
}

static_assert((kTpTaps & (kTpTaps - 1)) == 0, "the true-peak rings index with a mask");

// what one lookahead-limiter step needs from the lane's global ring; asked for ahead of the compressor's arithmetic
struct DynLimiterFetch {
  float delayed_in, sfx;
  int jn;  // the position after this step
};
__device__ __forceinline__ DynLimiterFetch dyn_limiter_fetch(const float *ring, const float *suf, int64_t LP, int j, int W) {
  DynLimiterFetch f;
  f.jn = (j + 1 == W) ? 0 : j + 1;
  f.delayed_in = ring[(int64_t)f.jn * LP];
  f.sfx = (j + 1 < W) ? suf[(int64_t)(j + 1) * LP] : 0.0f;
  return f;
}

struct DynLimiterState {
  double gain;
  float prefix;  // running prefix maximum of the current van-Herk block
};

// Limiter::process_sample, limiter.rs:246-284, at position j of the van-Herk block: returns delayed input * gain
__device__ __forceinline__ double dyn_limiter_step(float *ring, float *suf, int64_t LP, int j, int W, const DynLimiterFetch &f,
                                                   float xin, double ceil_lin, double rc, DynLimiterState &s, double &gmin) {
  const float ax = fabsf(xin);
  s.prefix = (j == 0) ? ax : fmaxf(s.prefix, ax);
  const double peak = (double)fmaxf(f.sfx, s.prefix);
  ring[(int64_t)j * LP] = xin;
  if (j + 1 == W) {  // block of W inputs complete: suffix maxima for the next block
    float m = 0.0f;
    for (int k = W - 1; k >= 0; --k) {
      m = fmaxf(m, fabsf(ring[(int64_t)k * LP]));
      suf[(int64_t)k * LP] = m;
    }
  }
  const double target = peak > ceil_lin ? ceil_lin / peak : 1.0;
  if (target < s.gain) {
    s.gain = target;
  } else {
    s.gain = rc * s.gain + (1.0 - rc) * target;
  }
  gmin = fmin(gmin, s.gain);
  return (double)f.delayed_in * s.gain;
}

struct DynTpStats {
  float in_peak, gmin;
  uint32_t limited;
};

// TruePeakLimiter::process_sample, true_peak.rs:337-378: `limited` is the lookahead limiter's product, t the sample index
__device__ __forceinline__ float dyn_tp_limiter_step(float (*tpi)[kLanes], int t, int lane, double limited, double ceil_lin,
                                                     float tp_ceiling, float rel, float &tp_gain, DynTpStats &st) {
  float input = (float)dclamp(limited, -ceil_lin, ceil_lin);
  if (!finite_f32(input)) input = 0.0f;
  tpi[t & (kTpTaps - 1)][lane] = input;
  const float delayed = tpi[(t - kTpDelay) & (kTpTaps - 1)][lane];
  const float itp = dyn_tp_observe(tpi, t, lane);
  st.in_peak = fmaxf(st.in_peak, itp);
  float tp_target = 1.0f;
  if (itp > tp_ceiling) tp_target = fclamp((tp_ceiling * 0.999f) / itp, 0.0f, 1.0f);
  if (tp_target < tp_gain) {
    tp_gain = tp_target;
    st.limited = 1;
  } else {
    tp_gain = rel * tp_gain + (1.0f - rel) * tp_target;
  }
  st.gmin = fminf(st.gmin, tp_gain);
  float o = fclamp(delayed * tp_gain, -tp_ceiling, tp_ceiling);
  if (!finite_f32(o)) o = 0.0f;
  return o;
}

struct DynOutputStats {
  double sq;
  float peak, tp;
  uint32_t non_finite;
};

// block output statistics + TruePeakDetector (block_processor.rs:158-159) for one output sample
__device__ __forceinline__ void dyn_output_observe(float (*tpo)[kLanes], int t, int lane, float o, DynOutputStats &st) {
  if (finite_f32(o)) {
    st.sq += (double)o * (double)o;
    tpo[t & (kTpTaps - 1)][lane] = o;
  } else {
    st.non_finite = 1;
    tpo[t & (kTpTaps - 1)][lane] = 0.0f;  // TruePeakDetector feeds 0 for non-finite, true_peak.rs:212
  }
  st.peak = fmaxf(st.peak, fabsf(o));
  st.tp = fmaxf(st.tp, dyn_tp_observe(tpo, t, lane));
}

// the limiter and true-peak fields of a row from a block's minima (limiter.rs:273-280; true_peak.rs:315-321, 363-365)
__device__ __forceinline__ float dyn_limiter_gr_db(double gmin) { return gmin < 1.0 ? (float)(-lin2db(gmin, 1e-10)) : 0.0f; }
__device__ __forceinline__ float dyn_tp_gr_db(float gmin) { return gmin < 1.0f ? -20.0f * log10f(fmaxf(gmin, 1e-10f)) : 0.0f; }

}  // namespace af
