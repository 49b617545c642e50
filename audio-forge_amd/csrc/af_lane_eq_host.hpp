// af_lane_eq_host.hpp -- records and the launcher the per-lane EQ (af_lane_eq.hip) shares with its host half
// (af_api_lane_eq.cpp).  A LANE is one (capture, band set) pair: it runs the 10-band EQ over its capture's row with its own
// section coefficients, from zero state.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "af_device.h"

namespace af {

constexpr int kLeSections = kNumBands;  // legacy (frequency, gain, Q) bands: a low shelf, eight bells, a high shelf, one section each

// what differs per lane, [field][padded lane]: the SectionParams of the lane's EqProto, section by section.
// f64 planes: section k's active b0 b1 b2 a1 a2 at 10 k + 0..4, its pending ones at 10 k + 5..9.
// i32 planes: section k's xf_total at 2 k, its xf_remaining at 2 k + 1.
constexpr int kLeCoefPlanes = 10 * kLeSections;
constexpr int kLeFadePlanes = 2 * kLeSections;

struct LaneEqArgs {
  const float *in;              // [captures][in_stride]
  float *out;                   // [lanes_padded][out_stride]
  const double *coef;           // [kLeCoefPlanes][lanes_padded]
  const int32_t *fade;          // [kLeFadePlanes][lanes_padded]
  const int32_t *lane_capture;  // [lanes_padded]; the padding repeats the last lane
  int64_t in_stride, out_stride, n_samples;
  int32_t n_lanes, lanes_padded;
};

hipError_t launch_lane_eq(const LaneEqArgs &args, hipStream_t stream);

}  // namespace af
