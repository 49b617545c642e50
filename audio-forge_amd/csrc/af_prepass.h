// af_prepass.h -- the device pieces the sample-serial pre-pass kernels share (af_prepass.hip), one copy of each role:
// the realtime front end, the suppressor's model-input roles, and the noise gate's detector and state machine.  The gate's
// integer logic (GateLogic) is also what gate_lane_kernel (af_gate.hip) steps.  Everything is forced inline: a kernel pays
// for exactly the roles it calls, with its own compile-time flags folded in.
#pragma once
#include <hip/hip_runtime.h>

#include "af_dsp.h"
#include "af_suppressor.h"

namespace af {

constexpr int kPreGroup = 64;           // streams per workgroup
constexpr int kPreRow = kPreGroup + 1;  // floats per LDS row: one sample of the 64 streams + a pad column

// samples of tile `ti` of an n-sample pass cut into tiles of T (the last one may be short)
template <int T>
__device__ __forceinline__ int tile_len(int64_t n, int64_t ti) {
  return (int)((n - ti * T) < T ? (n - ti * T) : T);
}
// the stream behind row r of the group that starts at s0: rows past the batch are clamped to its last stream, not skipped
__device__ __forceinline__ int row_of(const SuppArgs &a, int s0, int r) {
  return (s0 + r) < a.n_streams ? (s0 + r) : a.n_streams - 1;
}

// ------------------------------------------------------------------ the realtime front end, routing.rs:802-843
// State in the chain planes: DC block x1/y1 (f32), 80 Hz high-pass z1/z2 (f64).
struct FrontEnd {
  float dc_x1 = 0.0f, dc_y1 = 0.0f;
  double z1 = 0.0, z2 = 0.0;
  __device__ __forceinline__ void load(const SuppArgs &a, int64_t NS, int sc) {
    dc_x1 = a.chain_st32[(int64_t)a.f32_dc_x1 * NS + sc];
    dc_y1 = a.chain_st32[(int64_t)(a.f32_dc_x1 + 1) * NS + sc];
    z1 = a.chain_st64[(int64_t)a.f64_pre_z1 * NS + sc];
    z2 = a.chain_st64[(int64_t)(a.f64_pre_z1 + 1) * NS + sc];
  }
  __device__ __forceinline__ void store(const SuppArgs &a, int64_t NS, int s) const {
    a.chain_st32[(int64_t)a.f32_dc_x1 * NS + s] = dc_x1;
    a.chain_st32[(int64_t)(a.f32_dc_x1 + 1) * NS + s] = dc_y1;
    a.chain_st64[(int64_t)a.f64_pre_z1 * NS + s] = z1;
    a.chain_st64[(int64_t)(a.f64_pre_z1 + 1) * NS + s] = z2;
  }
  // one sample; hb0..ha2 are the high-pass's coefficients (SuppArgs::hp_*)
  __device__ __forceinline__ float step(float v, bool scrub, bool clamp, bool dc, bool hp_on, double hb0, double hb1, double hb2,
                                        double ha1, double ha2) {
    if (scrub && !finite_f32(v)) v = 0.0f;                       // routing.rs:808-811
    if (clamp) v = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);    // routing.rs:822
    if (dc) {                                                    // routing.rs:832-840
      const float o = v - dc_x1 + 0.995f * dc_y1;
      dc_x1 = v;
      dc_y1 = o;
      v = o;
      if (hp_on) {
        const double xin = (double)o;
        const double y = hb0 * xin + z1;
        z1 = hb1 * xin - ha1 * y + z2;
        z2 = hb2 * xin - ha2 * y;
        v = (float)y;
      }
    }
    return v;
  }
};

// ------------------------------------------------------------------ the suppressor's model input
// RNNoiseProcessor::scale_sample_for_model, rnnoise.rs:89-111
__device__ __forceinline__ float scale_for_model(float sample) {
  const float kScale = 32768.0f, kLimit = 32760.0f, kLimitUnit = 32760.0f / 32768.0f, kThr = 0.98f;
  const float kKnee = 1.0f - 0.98f;
  float v;
  if (!finite_f32(sample)) {
    v = 0.0f;
  } else {
    const float magnitude = fabsf(sample);
    if (magnitude <= kThr) {
      v = sample;
    } else {
      const float over = magnitude - kThr;
      const float compressed = over / (over + kKnee);
      const float softened = kThr + (kLimitUnit - kThr) * compressed;
      v = copysignf(fminf(softened, kLimitUnit), sample);
    }
  }
  const float scaled = v * kScale;
  return scaled < -kLimit ? -kLimit : (scaled > kLimit ? kLimit : scaled);
}

// RNNoise's own second-order input high-pass; its two memories live in SuppState::kHpMem
struct ModelHp {
  float m0 = 0.0f, m1 = 0.0f;
  __device__ __forceinline__ void load(const float *st) {
    m0 = st[SuppState::kHpMem];
    m1 = st[SuppState::kHpMem + 1];
  }
  __device__ __forceinline__ void store(float *st) const {
    st[SuppState::kHpMem] = m0;
    st[SuppState::kHpMem + 1] = m1;
  }
  __device__ __forceinline__ float step(float v) {
    const float b0 = -2.0f, b1 = 1.0f, a0 = -1.99599f, a1 = 0.99600f;
    const float y = v + m0;
    m0 = m1 + (b0 * v - a0 * y);
    m1 = (b1 * v - a1 * y);
    return y;
  }
};

// history: the previous 1728 model-input samples go in front of the window -- the tail of the previous window's buffer when
// there is one (its kernels may still be running), else what the last call saved.  Wave w copies rows w, w + n_waves, ...
template <int kUnroll>
__device__ __forceinline__ void copy_model_history(const SuppArgs &a, int s0, int wave, int n_waves, int lane, int64_t xh_stride) {
  for (int r = wave; r < kPreGroup; r += n_waves) {
    const int sr = row_of(a, s0, r);
    const float *hist = a.xh_prev ? a.xh_prev + (int64_t)sr * a.xh_prev_stride + (a.xh_prev_stride - kPitchBuf)
                                  : a.state + (int64_t)sr * SuppState::kCount + SuppState::kHist;
#pragma unroll kUnroll
    for (int i = lane; i < kPitchBuf; i += 64) a.xh[(int64_t)sr * xh_stride + i] = hist[i];
  }
}

// ------------------------------------------------------------------ lane = time roles
// A tile is T samples x 64 streams, rows of kRow floats.  Lane l works on sample l % T of rows (l / T) * T + r, r < T: a row
// segment is T x 4 bytes and a wave touches 64 / T rows per instruction.
// Model-input scaling of a tile: wrapper protocol, or raw (bin/rnnoise_benchmark.rs:75-79)
template <bool kRaw, int T, int kRow, int kUnroll>
__device__ __forceinline__ void scale_tile_for_model(const float *src, float *dst, int lane) {
  const int tl = lane & (T - 1), row0 = (lane / T) * T;
#pragma unroll kUnroll
  for (int r = 0; r < T; ++r) {
    float v = src[tl * kRow + row0 + r];
    if (kRaw) {
      v = (v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v)) * 32768.0f;
    } else {
      v = scale_for_model(v);
    }
    dst[tl * kRow + row0 + r] = v;
  }
}
// A tile's first `len` samples back to global rows: `dst` points at the tile's first sample in the row of stream 0
template <int T, int kRow, int kUnroll>
__device__ __forceinline__ void write_tile_rows(const float *src, float *dst, int64_t stride, int s0, int n_streams, int len, int lane) {
  const int tl = lane & (T - 1), row0 = (lane / T) * T;
#pragma unroll kUnroll
  for (int r = 0; r < T; ++r) {
    const int sr = s0 + row0 + r;
    if (sr < n_streams && tl < len) dst[(int64_t)sr * stride + tl] = src[tl * kRow + row0 + r];
  }
}

// ------------------------------------------------------------------ the noise gate, dsp/gate.rs
// R1, update_detector's envelope (gate.rs:266-270): the squared-RMS one-pole, row kGateRms of the gate state
struct GateDetector {
  double rms = 0.0;
  __device__ __forceinline__ void load(const int64_t *gs, int64_t NS, int sc) { rms = __longlong_as_double(gs[kGateRms * NS + sc]); }
  __device__ __forceinline__ void store(int64_t *gs, int64_t NS, int s) const { gs[kGateRms * NS + s] = __double_as_longlong(rms); }
  __device__ __forceinline__ double step(float x, double c, double omc) {
    const double xd = (double)x;
    rms = c * rms + omc * xd * xd;
    return rms;
  }
};

// F1 (lane = time): four waves of 16 streams each.  With T-sample tiles the 64 / T lane groups (grp = lane / T) share a
// wave's 16 rows: a lane takes gate_f1_rows(T) rows from gate_f1_row<T>.  The kernels' loops count j = 0 .. gate_f1_rows(T)
// and add the first row, so that the trip count is a constant: with `r < first + rows` as the bound, supp_prefilter_gate_kernel
// with the suppressor's roles compiled to 145 VGPRs (three waves per SIMD) instead of 114.
constexpr int gate_f1_rows(int T) { return 16 * T / 64; }
template <int T>
__device__ __forceinline__ int gate_f1_row(int f1_wave, int grp) { return f1_wave * 16 + grp * gate_f1_rows(T); }
// F1's level part.  `g` holds the detector's squared RMS and is left holding db_to_linear(-d), the gain the 4:1 expansion asks
// for at a depth of up to 36 dB (gate.rs:298-306); `level` is the detector level in dB (gate.rs:269).  Returns the decision
// bits: 1 level >= threshold, 2 level <= threshold - 4 dB, 4 depth beyond the 24 dB of the auto-relaxed range.
__device__ __forceinline__ int gate_level_part(double &g, double thr, double thr_low, double &level) {
  level = lin2db(sqrt(g), 1e-10);
  const double d = dclamp((thr - level) * (1.0 - 1.0 / 4.0), 0.0, 36.0);
  g = db2lin(-d);
  return (level >= thr ? 1 : 0) | (level <= thr_low ? 2 : 0) | (d > 24.0 ? 4 : 0);
}

// The gate's integer state and its per-sample steps: integers and comparisons only, the same for every kernel that gates.
struct GateLogic {
  int hold = 0, window = 0, trans = 0, cooldown = 0, relax = 0;
  bool open = false, eff = false, has_eff = false;
  int64_t events = 0;
  // update_detector's decision, gate.rs:271-285: threshold, hold, 4 dB hysteresis (bits 1 and 2 of gate_level_part)
  __device__ __forceinline__ void decide(int bits, int hold_samples) {
    if (bits & 1) {
      open = true;
      hold = hold_samples;
    } else if (hold > 0) {
      hold -= 1;
      open = true;
    } else if (bits & 2) {
      open = false;
    }
  }
  // track_gate_transition, gate.rs:590-623: four flips of the effective state inside the window are a chatter event, which
  // starts the cool-down and, where `arm_relax`, the auto-relaxed range
  __device__ __forceinline__ void track(bool effective_open, bool arm_relax, int window_samples, int cooldown_samples,
                                        int relax_samples) {
    if (!has_eff) {
      eff = effective_open;
      has_eff = true;
    } else if (effective_open != eff) {
      eff = effective_open;
      if (window == 0) {
        window = window_samples;
        trans = 1;
      } else {
        trans += 1;
      }
      if (trans >= 4 && cooldown == 0) {
        events += 1;
        cooldown = cooldown_samples;
        if (arm_relax) relax = relax_samples;
        window = 0;
        trans = 0;
      }
    }
  }
  // advance_chatter_timers, gate.rs:573-588
  __device__ __forceinline__ void advance_timers() {
    if (relax > 0) relax -= 1;
    if (window > 0) {
      window -= 1;
      if (window == 0) trans = 0;
    }
    if (cooldown > 0) cooldown -= 1;
  }
};

// R2 (lane = stream): the logic above with the smoothed linear gain, rows kGateGain .. kGateEvents of the gate state
struct GateCore : GateLogic {
  double gain = 0.0;
  __device__ __forceinline__ void load(const int64_t *gs, int64_t NS, int sc) {
    gain = __longlong_as_double(gs[kGateGain * NS + sc]);
    hold = (int)gs[kGateHold * NS + sc];
    window = (int)gs[kGateWindow * NS + sc];
    trans = (int)gs[kGateTrans * NS + sc];
    cooldown = (int)gs[kGateCooldown * NS + sc];
    relax = (int)gs[kGateRelax * NS + sc];
    open = gs[kGateOpen * NS + sc] != 0;
    eff = gs[kGateEff * NS + sc] != 0;
    has_eff = gs[kGateHasEff * NS + sc] != 0;
    events = gs[kGateEvents * NS + sc];
  }
  __device__ __forceinline__ void store(int64_t *gs, int64_t NS, int s) const {
    gs[kGateGain * NS + s] = __double_as_longlong(gain);
    gs[kGateHold * NS + s] = hold;
    gs[kGateWindow * NS + s] = window;
    gs[kGateTrans * NS + s] = trans;
    gs[kGateCooldown * NS + s] = cooldown;
    gs[kGateRelax * NS + s] = relax;
    gs[kGateOpen * NS + s] = open ? 1 : 0;
    gs[kGateEff * NS + s] = eff ? 1 : 0;
    gs[kGateHasEff * NS + s] = has_eff ? 1 : 0;
    gs[kGateEvents * NS + s] = events;
  }
  // apply_gain, gate.rs:625-635: attack / release smoothing towards the linear target, then the sample times the gain
  __device__ __forceinline__ float apply(float x, double target, const SuppArgs &a) {
    const bool up = target > gain;
    gain = (up ? a.gate_atk : a.gate_rel) * gain + (up ? a.gate_atk_omc : a.gate_rel_omc) * target;
    return (float)((double)x * gain);
  }
};

}  // namespace af
