// af_gate.hip -- the noise gate (rust-core/src/dsp/gate.rs) as the reference's offline operator uses it:
// `simulate_gate_suppressor_order` (python_api.rs:288-376) builds `NoiseGate::new(..)` + `set_gate_mode(VadAssisted)`
// without attaching a VadAutoGate, so `process_block_inplace` takes the per-sample downward-expander path
// (gate.rs:626-637): 8 ms RMS detector in dB, threshold / 4 dB hysteresis / 50 ms hold, 4:1 expansion capped at
// 36 dB (24 dB while the chatter auto-relax is active), one-pole attack/release on the linear gain, and the
// chatter detector (>= 4 open/close flips inside 500 ms, 1 s cool-down).  One recurrence per stream:
// lane per stream over 64 x 64 LDS tiles, state in registers.  The decision, the chatter tracking and its timers are
// GateLogic (af_prepass.h), the code the realtime gate stage steps; the f64 state rows, the detector and the smoothing are
// this kernel's own.
#include <hip/hip_runtime.h>

#include "af_dsp.h"
#include "af_prepass.h"

namespace af {

struct GateArgs {
  const float *in;
  float *out;
  float *gain_trace;      // [block][stream] current_gain at the end of every `block` samples, or null
  uint64_t *chatter;      // [stream] chatter events of this call (added to the state's count), or null
  double *state;          // [12][stream] persistent state, or null for a one-shot from the initial state
  double threshold_db, attack_coeff, release_coeff, rms_coeff;
  int64_t n_samples, stride;
  int32_t n_streams, block, vad_mode;
  int32_t hold_samples, window_samples, cooldown_samples, relax_samples;
};

__global__ __launch_bounds__(kLanes) void gate_lane_kernel(GateArgs a) {
  __shared__ float x[kTile][kLanes + 1];
  const int lane = threadIdx.x;
  const int s0 = blockIdx.x * kLanes;
  const int s = s0 + lane;
  const bool valid = s < a.n_streams;
  double rms = 0.0, gain = 0.0;
  GateLogic gl;  // (events: of this call)
  const int64_t NS = a.n_streams;
  if (a.state && valid) {
    rms = a.state[0 * NS + s]; gain = a.state[1 * NS + s];
    gl.hold = (int)a.state[2 * NS + s]; gl.window = (int)a.state[3 * NS + s]; gl.cooldown = (int)a.state[4 * NS + s];
    gl.relax = (int)a.state[5 * NS + s]; gl.trans = (int)a.state[6 * NS + s];
    gl.open = a.state[7 * NS + s] != 0.0; gl.eff = a.state[8 * NS + s] != 0.0; gl.has_eff = a.state[9 * NS + s] != 0.0;
  }
  int in_block = 0;
  int64_t block = 0;
  for (int64_t t0 = 0; t0 < a.n_samples; t0 += kTile) {
    const int len = (int)((a.n_samples - t0) < kTile ? (a.n_samples - t0) : kTile);
    for (int r = 0; r < kLanes; ++r) {
      const int sr = s0 + r;
      float v = 0.0f;
      if (sr < a.n_streams && lane < len) v = a.in[(int64_t)sr * a.stride + t0 + lane];
      x[lane][r] = v;
    }
    __syncthreads();
    for (int t = 0; t < len; ++t) {
      const double xin = (double)x[t][lane];
      // update_detector, gate.rs:265-285
      rms = a.rms_coeff * rms + (1.0 - a.rms_coeff) * xin * xin;
      const double level = lin2db(sqrt(rms), 1e-10);
      gl.decide((level >= a.threshold_db ? 1 : 0) | (level <= a.threshold_db - 4.0 ? 2 : 0), a.hold_samples);
      // detector_gain_reduction_db, gate.rs:288-306: the range is the one in force before this sample's transition is tracked
      const double range = gl.relax > 0 ? 24.0 : 36.0;
      const double gr = gl.open ? 0.0 : dclamp((a.threshold_db - level) * (1.0 - 1.0 / 4.0), 0.0, range);
      gl.track(gl.open, a.vad_mode != 0, a.window_samples, a.cooldown_samples, a.relax_samples);
      gl.advance_timers();
      // apply_gain, gate.rs:625-635
      const double target = db2lin(-gr);
      const double coeff = target > gain ? a.attack_coeff : a.release_coeff;
      gain = coeff * gain + (1.0 - coeff) * target;
      x[t][lane] = (float)(xin * gain);
      if (++in_block == a.block) {
        if (valid && a.gain_trace) a.gain_trace[block * NS + s] = (float)gain;
        in_block = 0;
        ++block;
      }
    }
    __syncthreads();
    for (int r = 0; r < kLanes; ++r) {
      const int sr = s0 + r;
      if (sr < a.n_streams && lane < len) a.out[(int64_t)sr * a.stride + t0 + lane] = x[lane][r];
    }
    __syncthreads();
  }
  if (valid) {
    if (in_block > 0 && a.gain_trace) a.gain_trace[block * NS + s] = (float)gain;
    if (a.chatter) a.chatter[s] = (uint64_t)gl.events;
    if (a.state) {
      a.state[0 * NS + s] = rms; a.state[1 * NS + s] = gain;
      a.state[2 * NS + s] = gl.hold; a.state[3 * NS + s] = gl.window; a.state[4 * NS + s] = gl.cooldown;
      a.state[5 * NS + s] = gl.relax; a.state[6 * NS + s] = gl.trans;
      a.state[7 * NS + s] = gl.open ? 1.0 : 0.0; a.state[8 * NS + s] = gl.eff ? 1.0 : 0.0; a.state[9 * NS + s] = gl.has_eff ? 1.0 : 0.0;
    }
  }
}

hipError_t launch_gate(const GateArgs &a, hipStream_t stream) {
  hipLaunchKernelGGL(gate_lane_kernel, dim3((a.n_streams + kLanes - 1) / kLanes), dim3(kLanes), 0, stream, a);
  return hipGetLastError();
}

}  // namespace af
