// af_compressor_search.hip -- the compressor calibration sweep: the dynamics half of the chain with PER-LANE compressor
// parameters over a shared input, and the fold of its per-block rows into one simulation record per lane.
//
// cs_sweep_kernel: a lane is one (capture, candidate) pair, a wave is 64 lanes.  Every lane runs what chain_lane_kernel
//   (af_kernels.hip) runs from the compressor on -- comp_sample with side chain, adaptive-release meter and block-end makeup
//   smoothing, the van-Herk lookahead limiter, the 4x true-peak limiter, output statistics and detector -- from zero state,
//   strictly sample-sequential, with the same operations in the same order: its rows equal the engine's bit for bit.
//   The input is read straight from the captures' rows (lanes of a wave that share a capture read one address; no transpose);
//   the two 32-tap true-peak histories are 32-row rings in LDS (16 KB per wave); the limiter's ring and suffix maxima are a
//   lane-major ring in global memory ([row][lane]: a wave's access is one 256 B line), so LDS does not bound the occupancy.
// cs_fold_kernel: one wave per lane folds the lane's rows and the capture's shared rows as python_api.rs:578-713 does
//   (mic_eq_core.chain_diagnostics): maxima, dB values, the percentiles of the gain-reduction traces and the pumping score.
//
// The per-sample dynamics step (compressor sample, limiter step, true-peak step, output observation, block-end makeup smoothing)
// is af_dynamics_step.h's, shared with the streaming lane chain (af_lane_chain.hip); af_kernels.hip keeps its own copy, so that
// file's code object is untouched.
#include <hip/hip_runtime.h>

#include "af_compressor_search_host.hpp"
#include "af_dsp.h"
#include "af_dynamics_step.h"

namespace af {

// =====================================================================================
// the sweep
// =====================================================================================
extern "C" __global__ __launch_bounds__(kLanes) void cs_sweep_kernel(CsSweepArgs a) {
  __shared__ float tpi[kTpTaps][kLanes];  // true-peak limiter input, last 32
  __shared__ float tpo[kTpTaps][kLanes];  // chain output, last 32

  const int lane = threadIdx.x;
  const int g = blockIdx.x * kLanes + lane;  // < lanes_padded: every per-lane array and the ring are padded to whole waves
  const bool valid = g < a.n_lanes;
  const int64_t LP = a.lanes_padded;
  const int W = a.lim.lookahead_samples + 1;
  float *ring = a.ring + g;                    // row r at ring[r * LP]
  float *suf = a.ring + (int64_t)W * LP + g;   // suffix maxima of the last complete block of W inputs

  CompressorParams P = a.uniform;
  P.threshold_db = a.lane_f64[(int64_t)kCsThresholdDb * LP + g];
  P.attack_coeff = a.lane_f64[(int64_t)kCsAttackCoeff * LP + g];
  P.detector_release_coeff = a.lane_f64[(int64_t)kCsDetectorReleaseCoeff * LP + g];
  P.base_release_ms = a.lane_f64[(int64_t)kCsBaseReleaseMs * LP + g];
  P.makeup_gain_db = a.lane_f64[(int64_t)kCsMakeupGainDb * LP + g];
  P.comp_factor = a.lane_f64[(int64_t)kCsCompFactor * LP + g];
  P.knee_start = a.lane_f64[(int64_t)kCsKneeStart * LP + g];
  P.knee_end = a.lane_f64[(int64_t)kCsKneeEnd * LP + g];
  const uint32_t lane_flags = a.lane_flags[g];
  P.adaptive_release = (lane_flags & kCsAdaptiveRelease) ? 1 : 0;
  P.sidechain_highpass_enabled = (lane_flags & kCsSidechainHighpass) ? 1 : 0;

  // a fresh processor: af_api.cpp, upload_initial_state
  DynCompState cs = {};
  cs.peak_env_db = -120.0;
  cs.cur_release_ms = a.lane_f64[(int64_t)kCsCurReleaseMs * LP + g];
  cs.target_release_ms = a.lane_f64[(int64_t)kCsTargetReleaseMs * LP + g];
  cs.release_coeff = a.lane_f64[(int64_t)kCsReleaseCoeff * LP + g];
  cs.smoothed_makeup = a.lane_f64[(int64_t)kCsSmoothedMakeup * LP + g];
  DynLimiterState lim = {1.0, 0.0f};
  float tp_gain = 1.0f;
  for (int r = 0; r < kTpTaps; ++r) {
    tpi[r][lane] = 0.0f;
    tpo[r][lane] = 0.0f;
  }
  __syncthreads();

  const float *in = a.in + (int64_t)a.lane_capture[g] * a.stride;
  float *audio = (a.audio && valid) ? a.audio + (int64_t)g * a.n_samples : nullptr;
  const double ceil_lin = a.lim.ceiling_linear;
  const double rc = a.lim.release_coeff;
  const float tp_ceiling = a.tp.ceiling_linear;
  const float rel = a.tp.release_coeff;
  const int cb = a.control_block;
  const int64_t n = a.n_samples;

  int j = 0;  // position in the van-Herk block of W inputs
  float x_next = n > 0 ? in[0] : 0.0f;
  int64_t block_index = 0;
  for (int64_t blk0 = 0; blk0 < n; blk0 += cb, ++block_index) {
    const int blk_len = (int)((n - blk0) < cb ? (n - blk0) : cb);
    DynTpStats tps = {0.0f, 1.0f, 0};
    DynOutputStats os = {0.0, 0.0f, 0.0f, 0};
    double lim_gmin = 1.0;
    const double makeup_lin = db2lin(cs.smoothed_makeup);  // constant inside a block (compressor.rs:771-772 vs 721)

    for (int i = 0; i < blk_len; ++i) {
      const int64_t t64 = blk0 + i;
      const int t = (int)(t64 & 0x7fffffff);  // only its low five bits are used
      // what this sample needs from memory, asked for ahead of the compressor's arithmetic
      const DynLimiterFetch lf = dyn_limiter_fetch(ring, suf, LP, j, W);
      const float x = x_next;
      x_next = (t64 + 1 < n) ? in[t64 + 1] : 0.0f;

      const float xin = dyn_comp_sample(P, cs, x, makeup_lin);                                             // compressor.rs:700-722
      const double limited = dyn_limiter_step(ring, suf, LP, j, W, lf, xin, ceil_lin, rc, lim, lim_gmin);  // limiter.rs:246-284
      j = lf.jn;
      const float o = dyn_tp_limiter_step(tpi, t, lane, limited, ceil_lin, tp_ceiling, rel, tp_gain, tps);  // true_peak.rs:337-378
      dyn_output_observe(tpo, t, lane, o, os);                                                             // block_processor.rs:158-159
      if (audio) audio[t64] = o;
    }

    dyn_block_end_makeup(P, cs, blk_len);
    if (valid) {
      CsRow st;
      st.output_sample_peak = os.peak;
      st.tp_limiter_input_peak = tps.in_peak;
      st.output_true_peak = os.tp;
      st.limiter_peak_gr_db = dyn_limiter_gr_db(lim_gmin);
      st.tp_limiter_gr_db = dyn_tp_gr_db(tps.gmin);
      st.compressor_gr_db = (float)cs.gr;
      st.makeup_gain_db = (float)cs.smoothed_makeup;
      st.pad = 0.0f;
      st.output_square_sum = os.sq;
      st.tp_limited_events = tps.limited;
      st.non_finite_output = os.non_finite;
      a.rows[block_index * a.n_lanes + g] = st;
    }
  }
}

// =====================================================================================
// the fold
// =====================================================================================
namespace {

// python_api.rs:54-56 in f32: 20 * log10(max(v, 1e-12)), the product rounded to f32.  The logarithm is taken in f64 and rounded
// once, i.e. the correctly rounded f32 log10 (a host libm's log10f is that value or its neighbour); the fold takes a few hundred
// per lane, so the f64 routine costs nothing.
__device__ __forceinline__ float cs_linear_to_db(float v) { return 20.0f * (float)log10((double)fmaxf(v, 1.0e-12f)); }

__device__ __forceinline__ float wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// python_api.rs:58-74 (mic_eq_core._percentile) over the elements of v[0..n) whose keep[] byte is set (keep == null: all of them):
// position in f32, floor and ceil, f32 lerp.  The two order statistics are found by rank (ties broken by index), which selects
// the elements a sort would put there.  Every thread of the wave calls it; `slot` is two floats of LDS.
__device__ float cs_percentile(const float *v, const uint8_t *keep, int n, int count, float pct, float *slot, int tid) {
  __syncthreads();
  if (count <= 0) return 0.0f;
  const float position = (float)(count - 1) * pct;
  const int lo = (int)floorf(position), hi = (int)ceilf(position);
  for (int i = tid; i < n; i += kLanes) {
    if (keep && !keep[i]) continue;
    const float x = v[i];
    int rank = 0;
    for (int k = 0; k < n; ++k) {
      if (keep && !keep[k]) continue;
      const float y = v[k];
      rank += (y < x || (y == x && k < i)) ? 1 : 0;
    }
    if (rank == lo) slot[0] = x;
    if (rank == hi) slot[1] = x;
  }
  __syncthreads();
  const float lower = slot[0], upper = slot[1];
  if (lo == hi) return lower;
  const float fraction = position - (float)lo;
  return lower + fraction * (upper - lower);
}

}  // namespace

extern "C" __global__ __launch_bounds__(kLanes) void cs_fold_kernel(CsFoldArgs a) {
  extern __shared__ double fold_lds[];  // [nb] f64, then three [nb] f32, then two [nb] u8
  __shared__ float slot[2];
  const int tid = threadIdx.x;
  const int lane = blockIdx.x;
  const int nb = a.n_blocks;
  double *out_sq = fold_lds;
  float *comp = reinterpret_cast<float *>(fold_lds + nb);  // max(compressor_gr_db, 0)
  float *va = comp + nb, *vb = va + nb;
  uint8_t *mask = reinterpret_cast<uint8_t *>(vb + nb), *keep = mask + nb;
  const int cap = a.lane_capture[lane];
  const CsCapture C = a.captures[cap];
  const float *in_db = a.in_db + (int64_t)cap * nb;
  const float *dees = a.deesser_db + (int64_t)cap * nb;
  const bool use_all = C.active_count < 3;  // python_api.rs:618-625
  const int active_count = use_all ? nb : C.active_count;

  // ---- maxima, counts, per-block levels
  float out_peak = 0.0f, tp_in_peak = 0.0f, out_tp = 0.0f, lim_gr = 0.0f, tp_gr = 0.0f, comp_gr = 0.0f;
  int events = 0, non_finite = 0, n_gain = 0, n_silence_level = 0, n_inactive = 0;
  for (int i = tid; i < nb; i += kLanes) {
    const CsRow r = a.rows[(int64_t)i * a.n_lanes + lane];
    out_peak = fmaxf(out_peak, r.output_sample_peak);
    tp_in_peak = fmaxf(tp_in_peak, r.tp_limiter_input_peak);
    out_tp = fmaxf(out_tp, r.output_true_peak);
    lim_gr = fmaxf(lim_gr, r.limiter_peak_gr_db);
    tp_gr = fmaxf(tp_gr, r.tp_limiter_gr_db);
    comp_gr = fmaxf(comp_gr, r.compressor_gr_db);
    events += (int)r.tp_limited_events;
    non_finite |= (int)r.non_finite_output;
    const int len = (int64_t)(i + 1) * a.control_block <= a.n_samples ? a.control_block : (int)(a.n_samples - (int64_t)i * a.control_block);
    out_sq[i] = r.output_square_sum;
    const float block_rms = (float)sqrt(r.output_square_sum / (double)len);
    comp[i] = r.compressor_gr_db > 0.0f ? r.compressor_gr_db : 0.0f;
    va[i] = cs_linear_to_db(block_rms) - in_db[i];  // out_db - in_db
    const uint8_t m = a.mask[(int64_t)cap * nb + i];
    mask[i] = m;
    n_gain += (m & (kCsActive | kCsAudible)) == (kCsActive | kCsAudible);
    n_silence_level += (m & (kCsActive | kCsAudible)) == kCsAudible;
    n_inactive += !(m & kCsActive);
  }
  out_peak = wave_max(out_peak); tp_in_peak = wave_max(tp_in_peak); out_tp = wave_max(out_tp);
  lim_gr = wave_max(lim_gr); tp_gr = wave_max(tp_gr); comp_gr = wave_max(comp_gr);
  events = wave_sum(events); non_finite = wave_sum(non_finite);
  n_gain = wave_sum(n_gain); n_silence_level = wave_sum(n_silence_level); n_inactive = wave_sum(n_inactive);
  __syncthreads();

  // ---- gain-reduction percentiles over the active blocks
  int n_above = 0;
  for (int i = tid; i < nb; i += kLanes) {
    keep[i] = use_all || (mask[i] & kCsActive);
    n_above += keep[i] && comp[i] >= 0.10f;
  }
  n_above = wave_sum(n_above);
  const float comp_median = cs_percentile(comp, keep, nb, active_count, 0.50f, slot, tid);
  const float comp_p95 = cs_percentile(comp, keep, nb, active_count, 0.95f, slot, tid);
  __syncthreads();
  for (int i = tid; i < nb; i += kLanes) vb[i] = dees[i] > 0.0f ? dees[i] : 0.0f;
  const float dees_median = cs_percentile(vb, keep, nb, active_count, 0.50f, slot, tid);
  const float dees_p95 = cs_percentile(vb, keep, nb, active_count, 0.95f, slot, tid);
  // ---- level medians
  __syncthreads();
  for (int i = tid; i < nb; i += kLanes) keep[i] = (mask[i] & (kCsActive | kCsAudible)) == (kCsActive | kCsAudible);
  const float active_output_gain = cs_percentile(va, keep, nb, n_gain, 0.50f, slot, tid);
  __syncthreads();
  for (int i = tid; i < nb; i += kLanes) keep[i] = (mask[i] & (kCsActive | kCsAudible)) == kCsAudible;
  const float silence_level_delta = cs_percentile(va, keep, nb, n_silence_level, 0.50f, slot, tid);
  __syncthreads();
  for (int i = tid; i < nb; i += kLanes) {
    keep[i] = !(mask[i] & kCsActive);
    vb[i] = -comp[i];
  }
  const float silence_output_gain = cs_percentile(vb, keep, nb, n_inactive, 0.50f, slot, tid);

  // ---- pumping score, python_api.rs:76-111 (mic_eq_core._pumping_score): the recurrence is serial
  __syncthreads();
  __shared__ int trace_bad;
  __shared__ double total_sq;
  if (tid == 0) {
    trace_bad = 0;
    double total = 0.0;
    for (int i = 0; i < nb; ++i) total += out_sq[i];  // the accumulation order of python_api.rs:519-571
    total_sq = total;
    if (nb >= 3) {
      float previous = comp[0], highpass = 0.0f, bandpass = 0.0f;
      for (int i = 1; i < nb; ++i) {
        const float value = comp[i];
        if (!finite_f32(value)) trace_bad = 1;
        highpass = a.highpass_alpha * (highpass + value - previous);
        bandpass = bandpass + a.lowpass_alpha * (highpass - bandpass);
        va[i - 1] = fabsf(bandpass);
        vb[i - 1] = fabsf(value - previous);
        previous = value;
      }
    }
  }
  float pumping = 0.0f;
  if (nb >= 3) {
    const float robust_limit = cs_percentile(va, nullptr, nb - 1, nb - 1, 0.95f, slot, tid);
    const float delta_p95 = cs_percentile(vb, nullptr, nb - 1, nb - 1, 0.95f, slot, tid);
    if (tid == 0) {
      float total = 0.0f;
      for (int i = 0; i < nb - 1; ++i) {
        const float v = fminf(va[i], robust_limit);
        total = total + v * v;
      }
      pumping = sqrtf(total / (float)(nb - 1)) + delta_p95;
      if (trace_bad) pumping = __builtin_inff();
    }
  }

  if (tid == 0) {
    af_chain_simulation r;
    const float ceiling = a.ceiling_db;
    const float output_rms = a.n_samples > 0 ? (float)sqrt(total_sq / (double)a.n_samples) : 0.0f;
    const float output_sample_peak_db = cs_linear_to_db(out_peak);
    const float pre_limiter_true_peak_db = cs_linear_to_db(tp_in_peak);
    const float output_true_peak_db = cs_linear_to_db(out_tp);
    r.input_sample_peak_db = cs_linear_to_db(C.input_sample_peak);
    r.input_rms_db = cs_linear_to_db(C.input_rms);
    r.output_sample_peak_db = output_sample_peak_db;
    r.pre_limiter_true_peak_db = pre_limiter_true_peak_db;
    r.output_true_peak_db = output_true_peak_db;
    r.output_rms_db = cs_linear_to_db(output_rms);
    r.limiter_effective_ceiling_db = ceiling;
    r.sample_headroom_db = ceiling - output_sample_peak_db;
    r.pre_limiter_true_peak_headroom_db = ceiling - pre_limiter_true_peak_db;
    r.true_peak_headroom_db = ceiling - output_true_peak_db;
    r.limiter_gain_reduction_db = lim_gr;
    r.true_peak_limiter_gain_reduction_db = tp_gr;
    r.true_peak_limited_events = (uint64_t)events;
    r.compressor_gain_reduction_db = comp_gr;
    r.deesser_gain_reduction_db = C.deesser_max_db;
    r.compressor_gain_reduction_median_db = comp_median;
    r.compressor_gain_reduction_p95_db = comp_p95;
    r.compressor_gain_reduction_active_ratio = active_count > 0 ? (float)n_above / (float)active_count : 0.0f;
    r.active_output_gain_db = active_output_gain;
    r.silence_output_gain_db = silence_output_gain;
    r.silence_level_delta_db = silence_level_delta;
    r.compressor_pumping_score_db = pumping;
    r.non_finite_output = non_finite ? 1 : 0;
    r.deesser_gain_reduction_median_db = dees_median;
    r.deesser_gain_reduction_p95_db = dees_p95;
    r.analysis_block_ms = 20.0f;
    r.active_analysis_threshold_db = C.active_threshold_db;
    r.active_analysis_block_count = (uint64_t)active_count;
    r.processed_samples = (uint64_t)a.n_samples;
    // raw maxima and selected elements, before any dB conversion
    r.output_sample_peak = out_peak;
    r.pre_limiter_true_peak = tp_in_peak;
    r.output_true_peak = out_tp;
    r.output_rms = output_rms;
    a.out[lane] = r;
  }
}

// ------------------------------------------------------------------ launchers
hipError_t launch_cs_sweep(const CsSweepArgs &args, hipStream_t stream) {
  hipLaunchKernelGGL(cs_sweep_kernel, dim3(args.lanes_padded / kLanes), dim3(kLanes), 0, stream, args);
  return hipGetLastError();
}

hipError_t launch_cs_fold(const CsFoldArgs &args, hipStream_t stream) {
  const size_t lds = (size_t)args.n_blocks * (sizeof(double) + 3 * sizeof(float) + 2);
  hipLaunchKernelGGL(cs_fold_kernel, dim3(args.n_lanes), dim3(kLanes), lds, stream, args);
  return hipGetLastError();
}

}  // namespace af
