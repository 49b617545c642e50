// af_retune.h -- the device half of live control: per-stream state edits of the reference's setters (af_retune.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "af_device.h"

namespace af {

// What a reference setter does to the RUNNING object beyond its parameters, as edits of f64 state-plane rows (F64Field,
// af_device.h).  Every kernel family -- lane, token ring, quad, the role kernels, the systolic EQ, the de-esser pass, the stage
// pipeline's serial stages -- loads these rows at the start of a launch and stores them at its end, so one edit serves all of
// them; the stage pipeline's rings hold signal histories only, which no setter touches.
enum RetuneKind : int32_t {
  kRetuneSet = 0,   // row[dst] := value
  kRetuneCopy = 1,  // row[dst] := row[src]   (e.g. "pending z := active z", biquad.rs:256-257)
  // rows[dst .. dst + 4] := the peaking coefficients b0 b1 b2 a1 a2 for cos(omega) = value, alpha = value2 and the gain in
  // row[src] dB: what Biquad::set_frequency / set_q schedule on a de-esser's dynamic EQ, whose gain is per-stream state
  kRetunePeaking = 2,
};
struct RetuneOp {
  int32_t kind, preset;  // only streams whose 64-stream group runs `preset` are touched
  int32_t dst, src;      // F64Field rows
  double value, value2;
};

struct RetuneArgs {
  const RetuneOp *ops;          // device, applied in order
  const int32_t *group_preset;  // device, [groups], or null (every group runs preset 0)
  double *st64;                 // [n_fields][n_streams]
  int32_t n_ops, n_streams, n_fields;
};
hipError_t launch_retune_state(const RetuneArgs &a, hipStream_t stream);

}  // namespace af
