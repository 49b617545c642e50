// af_lane_chain_host.hpp -- records and launchers the streaming lane chain (af_lane_chain.hip) shares with its host half
// (af_api_lane_chain.cpp).  A LANE is one stream: it runs input scrub -> 10-band EQ -> compressor -> lookahead limiter -> 4x
// true-peak limiter -> output statistics and detector under its OWN settings, and carries its state from call to call.
//
// Everything a lane owns lives in two planes, [row][padded lane], so that a wave's access to one row is one line:
//   p64 (f64)   coefficients, filter memories, compressor state, limiter gain, then the lane's f64 parameters;
//   p32 (32-bit words: i32, u32 or f32 by row)   crossfade counters, stage flags, f32 parameters, true-peak gain, limiter
//               prefix maximum, the two 32-tap true-peak histories, then the limiter's delay ring and suffix maxima.
// What is NOT per lane: the position in the van-Herk block and the low bits of the sample index the 32-row histories are
// addressed with.  Both are the object's (samples processed by the object so far, modulo W and modulo 32), wave-uniform:
// a lane configured later starts with zero rings, and the maximum over the last W inputs, the W-1 sample delay and the FIR
// over the last 32 inputs do not depend on where in a zeroed ring a lane starts.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "af_device.h"

namespace af {

constexpr int kLcSections = kNumBands;  // legacy (frequency, gain, Q) bands: one section each

// ---- p64 rows
enum LcF64Row : int {
  kLcCoef = 0,                            // section k: active b0 b1 b2 a1 a2 at 10 k + 0..4, pending at 10 k + 5..9
  kLcEqMem = kLcCoef + 10 * kLcSections,  // section k: z1 z2 pz1 pz2 at 4 k + 0..3
  kLcComp = kLcEqMem + 4 * kLcSections,   // DynCompState, 15 rows in declaration order
  kLcLimGain = kLcComp + 15,
  // parameters (written by configure only): the doubles CompressorProto::params() and LimiterProto::params() give the engine
  kLcThresholdDb, kLcAttackCoeff, kLcDetectorReleaseCoeff, kLcBaseReleaseMs, kLcMakeupGainDb, kLcCompFactor, kLcKneeStart,
  kLcKneeEnd, kLcLimCeilingLinear, kLcLimReleaseCoeff,
  kLcF64Rows
};
// ---- p32 rows
enum LcF32Row : int {
  kLcFade = 0,                             // i32; section k: xf_total at 2 k, xf_remaining at 2 k + 1
  kLcFlags = kLcFade + 2 * kLcSections,    // u32, LcFlag
  kLcTpCeiling, kLcTpReleaseCoeff,         // f32 parameters (TruePeakProto)
  kLcTpGain, kLcLimPrefix,                 // f32 state
  kLcTpInHist,                             // 32 rows, row (t & 31) holds sample t
  kLcTpOutHist = kLcTpInHist + kTpTaps,
  kLcRing = kLcTpOutHist + kTpTaps,        // W rows delay ring, then W rows suffix maxima, W = lookahead + 1
  kLcF32Fixed = kLcRing
};
inline int lc_f32_rows(int lookahead) { return kLcF32Fixed + 2 * (lookahead + 1); }

enum LcFlag : uint32_t {
  kLcEqOn = 1u << 0, kLcCompressorOn = 1u << 1, kLcLimiterOn = 1u << 2, kLcAdaptiveRelease = 1u << 3, kLcSidechainHighpass = 1u << 4
};

struct LaneChainArgs {
  const float *in;           // [n_lanes][stride]
  float *out;                // [n_lanes][stride]
  double *p64;               // [kLcF64Rows][lanes_padded]
  uint32_t *p32;             // [lc_f32_rows(lookahead)][lanes_padded]
  BlockStats *rows;          // [blocks][n_lanes]
  CompressorParams uniform;  // the fields every lane shares (they depend on the sample rate alone)
  int64_t stride, n_samples;
  int64_t samples_before;    // processed by the object before this call: phase of the 32-row histories
  int32_t n_lanes, lanes_padded, control_block, lookahead_samples;
  int32_t ring_position;     // samples_before % (lookahead_samples + 1)
  int32_t pad;
};

// configure / reset: column i of the packed records becomes lane streams[i]'s rows; its rings are zeroed
struct LaneChainScatterArgs {
  const double *col64;     // [n][kLcF64Rows]
  const uint32_t *col32;   // [n][kLcF32Fixed]
  const int32_t *streams;  // [n] lanes, each < lanes_padded
  double *p64;
  uint32_t *p32;
  int32_t n, lanes_padded, f32_rows, pad;
};

hipError_t launch_lane_chain(const LaneChainArgs &args, hipStream_t stream);
hipError_t launch_lane_chain_scatter(const LaneChainScatterArgs &args, hipStream_t stream);

}  // namespace af
