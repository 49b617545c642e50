// af_lane_chain.hip -- the streaming lane chain: one stream per lane, every lane under its own settings, state carried from
// call to call.
//
// lane_chain_kernel: a wave is 64 streams, a workgroup is one wave.  Per control block and 64-sample tile a lane runs
//   input scrub and block input statistics -> the ten-band EQ with its own coefficients (lane_eq_kernel's two forms: band-major
//   with the parallel-state crossfade while some lane of the wave still crossfades, sample-major with the ten sections unrolled
//   afterwards) -> the dynamics step of af_dynamics_step.h with its own compressor and limiter parameters -> the tile's output.
//   ONE fused kernel, in two register phases per tile: the EQ's 50 coefficients and 20 memories (140 VGPRs) pass through
//   registers for one tile and live in the planes otherwise, so they are not live across the dynamics loop, whose 15
//   compressor doubles, ten parameters and 32-tap FIR window are; both sets held for the whole call do not fit the register
//   file.  As built: 256 VGPRs and 246 AGPRs (502 of the wave's 512 unified registers, occupancy 1), 8 VGPRs and 88 SGPRs
//   spilled into registers, no scratch -- at the ceiling: growth in af_dynamics_step.h will reach scratch.
//   A wave per SIMD is all the occupancy a latency-bound, sample-sequential lane can use; the two-kernel form would add a
//   [lanes][n] round trip through memory and a second launch for nothing.
//   The arithmetic is chain_lane_kernel's (af_kernels.hip), strictly sample-sequential per lane: f64 DF2T rounded to f32 after
//   every section, the compressor, limiter and true-peak steps as the sweep runs them.  Stage enables are per lane: a lane
//   with its EQ, compressor or limiter stage off skips that stage and leaves its state alone; a lane without the limiter
//   stage has no lookahead delay.
//   Audio moves through a 64 x 65 f32 LDS tile in both directions (256 B of one stream's row per instruction); the 32-tap
//   true-peak histories are 32-row rings in LDS, loaded from and stored to the planes once per call; the limiter's ring and
//   suffix maxima stay in the planes.  Padded lanes of a last partial wave compute on zeros inside the planes' padding and
//   touch neither the caller's input nor its output nor the rows.
// lane_chain_scatter_kernel: configure / reset.  One workgroup per listed stream copies the stream's packed column into the
//   planes and zeroes its limiter rings; no other lane's rows are touched.
#include <hip/hip_runtime.h>

#include "af_dsp.h"
#include "af_dynamics_step.h"
#include "af_lane_chain_host.hpp"

namespace af {

namespace {

// stream rows -> tile, transposed; non-finite input is zeroed as the engine does (python_api.rs:517-520)
__device__ __forceinline__ void lc_load_tile(const LaneChainArgs &a, float (*x)[kLanes + 1], int64_t t0, int len, int g0, int lane) {
#pragma unroll 8
  for (int r = 0; r < kLanes; ++r) {
    float v = 0.0f;
    if (g0 + r < a.n_lanes && lane < len) v = a.in[(int64_t)(g0 + r) * a.stride + t0 + lane];
    if (!finite_f32(v)) v = 0.0f;
    x[lane][r] = v;
  }
  __syncthreads();
}

// tile -> output rows: 256 B of one stream's row per instruction; never a padded lane's
__device__ __forceinline__ void lc_store_tile(const LaneChainArgs &a, float (*x)[kLanes + 1], int64_t t0, int len, int g0, int lane) {
  __syncthreads();
  if (lane < len) {
#pragma unroll 8
    for (int r = 0; r < kLanes; ++r)
      if (g0 + r < a.n_lanes) a.out[(int64_t)(g0 + r) * a.stride + t0 + lane] = x[lane][r];
  }
  __syncthreads();
}

// One tile of the EQ for a lane that may crossfade (Biquad::process_sample, biquad.rs:263-327): band-major like the engine, the
// crossfade position per lane and per section.  Coefficients, memories and counters come from the planes and go back to them;
// returns whether the lane still crossfades.
__device__ __forceinline__ bool lc_eq_tile_crossfade(double *p64, uint32_t *p32, int64_t LP, float (*x)[kLanes + 1], int len, int lane) {
  bool fading = false;
#pragma nounroll
  for (int k = 0; k < kLcSections; ++k) {
    double *f = p64 + (int64_t)(kLcCoef + 10 * k) * LP;
    double *m = p64 + (int64_t)(kLcEqMem + 4 * k) * LP;
    BiquadCoef c{f[0], f[LP], f[2 * LP], f[3 * LP], f[4 * LP]};
    const BiquadCoef p{f[5 * LP], f[6 * LP], f[7 * LP], f[8 * LP], f[9 * LP]};
    double z1 = m[0], z2 = m[LP], pz1 = m[2 * LP], pz2 = m[3 * LP];
    const int xf_total = (int)p32[(int64_t)(kLcFade + 2 * k) * LP];
    int rem = (int)p32[(int64_t)(kLcFade + 2 * k + 1) * LP];
    const double total = (double)xf_total;
#pragma nounroll
    for (int t = 0; t < len; ++t) {
      const double in = (double)x[t][lane];
      double y;
      if (rem > 0) {
        const double ya = c.b0 * in + z1;
        z1 = c.b1 * in - c.a1 * ya + z2;
        z2 = c.b2 * in - c.a2 * ya;
        const double yp = p.b0 * in + pz1;
        pz1 = p.b1 * in - p.a1 * yp + pz2;
        pz2 = p.b2 * in - p.a2 * yp;
        const int fade_pos = xf_total - rem + 1;
        const double fade = (double)fade_pos / total;
        y = ya * (1.0 - fade) + yp * fade;
        rem -= 1;
        if (rem == 0) {  // promote_pending_coefficients, biquad.rs:276-286
          c = p;
          z1 = pz1;
          z2 = pz2;
        }
      } else {
        y = c.b0 * in + z1;
        z1 = c.b1 * in - c.a1 * y + z2;
        z2 = c.b2 * in - c.a2 * y;
      }
      x[t][lane] = (float)y;
    }
    f[0] = c.b0; f[LP] = c.b1; f[2 * LP] = c.b2; f[3 * LP] = c.a1; f[4 * LP] = c.a2;
    m[0] = z1; m[LP] = z2; m[2 * LP] = pz1; m[3 * LP] = pz2;
    p32[(int64_t)(kLcFade + 2 * k + 1) * LP] = (uint32_t)rem;
    fading |= rem > 0;
  }
  return fading;
}

// One tile of the EQ for a lane that does not crossfade: sample-major with the ten sections unrolled, 50 coefficients and 20
// memories in registers for the tile, which leaves the compiler section k's memory updates to fill the latency of section
// k+1's dependent chain.  A section's output depends only on its own input sequence, so both orders give the same bits.
__device__ __forceinline__ void lc_eq_tile_steady(double *p64, int64_t LP, float (*x)[kLanes + 1], int len, int lane) {
  BiquadCoef c[kLcSections];
  double z1[kLcSections], z2[kLcSections];
#pragma unroll
  for (int k = 0; k < kLcSections; ++k) {
    const double *f = p64 + (int64_t)(kLcCoef + 10 * k) * LP;
    c[k] = BiquadCoef{f[0], f[LP], f[2 * LP], f[3 * LP], f[4 * LP]};
    z1[k] = p64[(int64_t)(kLcEqMem + 4 * k) * LP];
    z2[k] = p64[(int64_t)(kLcEqMem + 4 * k + 1) * LP];
  }
#pragma nounroll
  for (int t = 0; t < len; ++t) {
    float v = x[t][lane];
#pragma unroll
    for (int k = 0; k < kLcSections; ++k) {
      const double in = (double)v;
      const double y = c[k].b0 * in + z1[k];
      z1[k] = c[k].b1 * in - c[k].a1 * y + z2[k];
      z2[k] = c[k].b2 * in - c[k].a2 * y;
      v = (float)y;
    }
    x[t][lane] = v;
  }
#pragma unroll
  for (int k = 0; k < kLcSections; ++k) {
    p64[(int64_t)(kLcEqMem + 4 * k) * LP] = z1[k];
    p64[(int64_t)(kLcEqMem + 4 * k + 1) * LP] = z2[k];
  }
}

}  // namespace

extern "C" __global__ __launch_bounds__(kLanes) void lane_chain_kernel(LaneChainArgs a) {
  __shared__ float x[kTile][kLanes + 1];
  __shared__ float tpi[kTpTaps][kLanes];  // true-peak limiter input, last 32
  __shared__ float tpo[kTpTaps][kLanes];  // chain output, last 32

  const int lane = threadIdx.x;
  const int g0 = blockIdx.x * kLanes;
  const int g = g0 + lane;  // < lanes_padded: every plane is padded to whole waves
  const bool valid = g < a.n_lanes;
  const int64_t LP = a.lanes_padded;
  const int W = a.lookahead_samples + 1;
  double *p64 = a.p64 + g;      // row r at p64[r * LP]
  uint32_t *p32 = a.p32 + g;    // row r at p32[r * LP]
  float *ring = reinterpret_cast<float *>(p32) + (int64_t)kLcRing * LP;
  float *suf = ring + (int64_t)W * LP;  // suffix maxima of the last complete block of W inputs

  // ---- the lane's parameters
  const uint32_t flags = p32[(int64_t)kLcFlags * LP];
  const bool eq_on = (flags & kLcEqOn) != 0, comp_on = (flags & kLcCompressorOn) != 0, lim_on = (flags & kLcLimiterOn) != 0;
  CompressorParams P = a.uniform;
  P.threshold_db = p64[(int64_t)kLcThresholdDb * LP];
  P.attack_coeff = p64[(int64_t)kLcAttackCoeff * LP];
  P.detector_release_coeff = p64[(int64_t)kLcDetectorReleaseCoeff * LP];
  P.base_release_ms = p64[(int64_t)kLcBaseReleaseMs * LP];
  P.makeup_gain_db = p64[(int64_t)kLcMakeupGainDb * LP];
  P.comp_factor = p64[(int64_t)kLcCompFactor * LP];
  P.knee_start = p64[(int64_t)kLcKneeStart * LP];
  P.knee_end = p64[(int64_t)kLcKneeEnd * LP];
  P.adaptive_release = (flags & kLcAdaptiveRelease) ? 1 : 0;
  P.sidechain_highpass_enabled = (flags & kLcSidechainHighpass) ? 1 : 0;
  const double ceil_lin = p64[(int64_t)kLcLimCeilingLinear * LP];
  const double rc = p64[(int64_t)kLcLimReleaseCoeff * LP];
  const float tp_ceiling = __uint_as_float(p32[(int64_t)kLcTpCeiling * LP]);
  const float rel = __uint_as_float(p32[(int64_t)kLcTpReleaseCoeff * LP]);

  // ---- the lane's state.  The EQ's coefficients, memories and crossfade counters stay in the planes and pass through
  //      registers one tile at a time (lc_eq_tile), so that they are not live across the dynamics loop; only whether the lane
  //      still crossfades is carried.
  bool fading = false;
#pragma unroll
  for (int k = 0; k < kLcSections; ++k) fading |= (int)p32[(int64_t)(kLcFade + 2 * k + 1) * LP] > 0;
  fading = fading && eq_on;
  DynCompState cs;
  {
    const double *f = p64 + (int64_t)kLcComp * LP;
    cs.sc_prev_in = f[0]; cs.sc_prev_out = f[LP]; cs.low_env = f[2 * LP]; cs.voiced_env = f[3 * LP];
    cs.presence_env = f[4 * LP]; cs.plosive = f[5 * LP]; cs.peak_env_db = f[6 * LP]; cs.rms_env_sq = f[7 * LP];
    cs.gr = f[8 * LP]; cs.fast_env = f[9 * LP]; cs.slow_env = f[10 * LP]; cs.cur_release_ms = f[11 * LP];
    cs.target_release_ms = f[12 * LP]; cs.release_coeff = f[13 * LP]; cs.smoothed_makeup = f[14 * LP];
  }
  DynLimiterState lim;
  lim.gain = p64[(int64_t)kLcLimGain * LP];
  lim.prefix = __uint_as_float(p32[(int64_t)kLcLimPrefix * LP]);
  float tp_gain = __uint_as_float(p32[(int64_t)kLcTpGain * LP]);
  for (int r = 0; r < kTpTaps; ++r) {
    tpi[r][lane] = __uint_as_float(p32[(int64_t)(kLcTpInHist + r) * LP]);
    tpo[r][lane] = __uint_as_float(p32[(int64_t)(kLcTpOutHist + r) * LP]);
  }
  __syncthreads();

  const int cb = a.control_block;
  const int64_t n = a.n_samples;
  int j = a.ring_position;  // position in the van-Herk block of W inputs, wave-uniform
  int64_t block_index = 0;
  for (int64_t blk0 = 0; blk0 < n; blk0 += cb, ++block_index) {
    const int blk_len = (int)((n - blk0) < cb ? (n - blk0) : cb);
    float in_peak = 0.0f;
    double in_sq = 0.0, lim_gmin = 1.0;
    DynTpStats tps = {0.0f, 1.0f, 0};
    DynOutputStats os = {0.0, 0.0f, 0.0f, 0};
    const double makeup_lin = db2lin(cs.smoothed_makeup);  // constant inside a block (compressor.rs:771-772 vs 721)

    for (int t0 = 0; t0 < blk_len; t0 += kTile) {
      const int len = (blk_len - t0) < kTile ? (blk_len - t0) : kTile;
      const int64_t abs0 = blk0 + t0;
      lc_load_tile(a, x, abs0, len, g0, lane);

      // ---- block input statistics, on the scrubbed input (python_api.rs:515-523)
      for (int t = 0; t < len; ++t) {
        const float v = x[t][lane];
        in_sq += (double)v * (double)v;
        in_peak = fmaxf(in_peak, fabsf(v));
      }

      // ---- ten-band EQ (eq.rs:371-379): band-major while some lane of the wave crossfades, else sample-major
      if (__ballot(fading) != 0) {
        if (eq_on) fading = lc_eq_tile_crossfade(p64, p32, LP, x, len, lane);
      } else if (eq_on) {
        lc_eq_tile_steady(p64, LP, x, len, lane);
      }

      // ---- dynamics, sample by sample (af_dynamics_step.h)
      const int64_t phase0 = a.samples_before + abs0;
#pragma nounroll
      for (int t = 0; t < len; ++t) {
        const int ts = (int)((phase0 + t) & 0x7fffffff);  // only its low five bits are used
        // what this sample needs from the limiter's ring, asked for ahead of the compressor's arithmetic
        const DynLimiterFetch lf = dyn_limiter_fetch(ring, suf, LP, j, W);
        float v = x[t][lane];
        if (comp_on) v = dyn_comp_sample(P, cs, v, makeup_lin);  // compressor.rs:700-722
        float o = v;
        if (lim_on) {
          const double limited = dyn_limiter_step(ring, suf, LP, j, W, lf, v, ceil_lin, rc, lim, lim_gmin);  // limiter.rs:246-284
          o = dyn_tp_limiter_step(tpi, ts, lane, limited, ceil_lin, tp_ceiling, rel, tp_gain, tps);          // true_peak.rs:337-378
        }
        j = lf.jn;
        dyn_output_observe(tpo, ts, lane, o, os);  // block_processor.rs:158-159
        x[t][lane] = o;
      }
      lc_store_tile(a, x, abs0, len, g0, lane);
    }

    // ---- end of block
    if (comp_on) {
      dyn_block_end_makeup(P, cs, blk_len);
    } else {
      cs.gr = 0.0;  // compressor.rs:705-708
    }
    if (valid) {
      BlockStats st;
      st.input_sample_peak = in_peak;
      st.output_sample_peak = os.peak;
      st.tp_limiter_input_peak = tps.in_peak;
      st.output_true_peak = os.tp;
      st.limiter_peak_gr_db = dyn_limiter_gr_db(lim_gmin);  // (1 and 0 dB with the limiter stage off)
      st.tp_limiter_gr_db = dyn_tp_gr_db(tps.gmin);
      st.compressor_gr_db = comp_on ? (float)cs.gr : 0.0f;
      st.deesser_gr_db = 0.0f;
      st.input_square_sum = in_sq;
      st.output_square_sum = os.sq;
      st.tp_limited_events = tps.limited;
      st.non_finite_output = os.non_finite;
      st.makeup_gain_db = comp_on ? (float)cs.smoothed_makeup : 0.0f;
      st.makeup_activity = 0.0f;
      st.makeup_reliability = 0.0f;
      st.pad = 0.0f;
      a.rows[block_index * a.n_lanes + g] = st;
    }
  }

  // ---- save the lane's state (a padded lane's goes to the planes' padding)
  {
    double *f = p64 + (int64_t)kLcComp * LP;
    f[0] = cs.sc_prev_in; f[LP] = cs.sc_prev_out; f[2 * LP] = cs.low_env; f[3 * LP] = cs.voiced_env;
    f[4 * LP] = cs.presence_env; f[5 * LP] = cs.plosive; f[6 * LP] = cs.peak_env_db; f[7 * LP] = cs.rms_env_sq;
    f[8 * LP] = cs.gr; f[9 * LP] = cs.fast_env; f[10 * LP] = cs.slow_env; f[11 * LP] = cs.cur_release_ms;
    f[12 * LP] = cs.target_release_ms; f[13 * LP] = cs.release_coeff; f[14 * LP] = cs.smoothed_makeup;
  }
  p64[(int64_t)kLcLimGain * LP] = lim.gain;
  p32[(int64_t)kLcLimPrefix * LP] = __float_as_uint(lim.prefix);
  p32[(int64_t)kLcTpGain * LP] = __float_as_uint(tp_gain);
  for (int r = 0; r < kTpTaps; ++r) {
    p32[(int64_t)(kLcTpInHist + r) * LP] = __float_as_uint(tpi[r][lane]);
    p32[(int64_t)(kLcTpOutHist + r) * LP] = __float_as_uint(tpo[r][lane]);
  }
}

extern "C" __global__ __launch_bounds__(128) void lane_chain_scatter_kernel(LaneChainScatterArgs a) {
  const int i = blockIdx.x;  // < a.n
  const int64_t LP = a.lanes_padded;
  const int s = a.streams[i];
  if (s < 0 || s >= a.lanes_padded) return;  // (the host checks; never expected)
  for (int r = threadIdx.x; r < kLcF64Rows; r += blockDim.x) a.p64[(int64_t)r * LP + s] = a.col64[(int64_t)i * kLcF64Rows + r];
  for (int r = threadIdx.x; r < a.f32_rows; r += blockDim.x)
    a.p32[(int64_t)r * LP + s] = r < kLcF32Fixed ? a.col32[(int64_t)i * kLcF32Fixed + r] : 0u;  // zeroed limiter rings
}

// ------------------------------------------------------------------ launchers
hipError_t launch_lane_chain(const LaneChainArgs &args, hipStream_t stream) {
  hipLaunchKernelGGL(lane_chain_kernel, dim3(args.lanes_padded / kLanes), dim3(kLanes), 0, stream, args);
  return hipGetLastError();
}

hipError_t launch_lane_chain_scatter(const LaneChainScatterArgs &args, hipStream_t stream) {
  hipLaunchKernelGGL(lane_chain_scatter_kernel, dim3(args.n), dim3(128), 0, stream, args);
  return hipGetLastError();
}

}  // namespace af
