// af_compressor_search_host.hpp -- records and launchers the compressor candidate sweep (af_compressor_search.hip) shares with
// its host half (af_api_compressor_search.cpp).  A LANE is one (capture, candidate) pair: it runs the dynamics half of the
// chain (compressor -> lookahead limiter -> 4x true-peak limiter -> output statistics) over its capture's compressor input.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/audioforge_mi.h"
#include "af_device.h"

namespace af {

constexpr int kCsMaxBlocks = 2048;  // control blocks per capture the fold sizes its LDS for (40.96 s at 48 kHz)

// what differs per lane, as f64 planes [field][padded lane]: the candidate's share of CompressorParams (exactly the doubles
// CompressorProto::params() gives the engine) and the four state values a fresh compressor does not start at zero with
enum CsLaneField : int {
  kCsThresholdDb = 0, kCsAttackCoeff, kCsDetectorReleaseCoeff, kCsBaseReleaseMs, kCsMakeupGainDb, kCsCompFactor, kCsKneeStart,
  kCsKneeEnd, kCsCurReleaseMs, kCsTargetReleaseMs, kCsReleaseCoeff, kCsSmoothedMakeup, kCsLaneFields
};
enum CsLaneFlag : uint32_t { kCsAdaptiveRelease = 1u << 0, kCsSidechainHighpass = 1u << 1 };

// the candidate-dependent fields of BlockStats, one per control block and lane
struct CsRow {
  float output_sample_peak, tp_limiter_input_peak, output_true_peak;
  float limiter_peak_gr_db, tp_limiter_gr_db, compressor_gr_db, makeup_gain_db, pad;
  double output_square_sum;
  uint32_t tp_limited_events, non_finite_output;
};

struct CsSweepArgs {
  const float *in;              // [captures][stride] compressor input
  const double *lane_f64;       // [kCsLaneFields][lanes_padded]
  const int32_t *lane_capture;  // [lanes_padded]
  const uint32_t *lane_flags;   // [lanes_padded] CsLaneFlag
  float *ring;                  // [2 * (lookahead + 1)][lanes_padded], zero: the limiter's delay ring, then its suffix maxima
  CsRow *rows;                  // [blocks][n_lanes]
  float *audio;                 // null, or [n_lanes][n_samples]
  CompressorParams uniform;     // the fields every lane shares (per-lane ones are overwritten in the kernel)
  LimiterParams lim;
  TruePeakParams tp;
  int64_t stride, n_samples;
  int32_t n_lanes, lanes_padded, control_block, pad;
};

// per capture, from the host (O(blocks) in f32/f64: af_compressor_search_math.h)
struct CsCapture {
  float input_sample_peak, input_rms, active_threshold_db, deesser_max_db;
  int32_t active_count, pad;
};
enum CsMaskBit : uint8_t { kCsActive = 1, kCsAudible = 2 };

struct CsFoldArgs {
  const CsRow *rows;            // [blocks][n_lanes]
  const int32_t *lane_capture;  // [n_lanes]
  const float *in_db;           // [captures][n_blocks]
  const float *deesser_db;      // [captures][n_blocks]
  const uint8_t *mask;          // [captures][n_blocks] CsMaskBit
  const CsCapture *captures;
  af_chain_simulation *out;     // [n_lanes]
  int64_t n_samples;
  int32_t n_lanes, n_blocks, control_block;
  float ceiling_db, highpass_alpha, lowpass_alpha;
};

hipError_t launch_cs_sweep(const CsSweepArgs &args, hipStream_t stream);
hipError_t launch_cs_fold(const CsFoldArgs &args, hipStream_t stream);

}  // namespace af
