// af_output_writer_host.hpp -- what the host side and the kernels of the output writer (af_output_writer.hip) share: the
// constants of rust-core/src/audio/processor.rs:66-70 and dsp_loop.rs:781-795, the state plane's fields and the launchers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace af {

constexpr int kOwMaxBlock = 8192;        // frames per push: the realtime path's blocks stay below the 8672-frame scratches
constexpr int kOwScratch = 8672;         // OUTPUT_QUEUE_CONTROL_CAPACITY and its two siblings, dsp_loop.rs
constexpr int kOwTaps = 32;              // TRUE_PEAK_TAPS_PER_PHASE, true_peak.rs
constexpr int kOwLookahead = 20;         // TRUE_PEAK_LIMITER_LOOKAHEAD_SAMPLES, true_peak.rs
constexpr float kOwRatioAdjust = 0.008f;    // OUTPUT_DRIFT_MAX_RATIO_ADJUST, processor.rs:69
constexpr float kOwMinRatio = 0.96f;        // OUTPUT_DRIFT_MAX_EXPANSION_RATIO, processor.rs:70
constexpr float kOwMaxCatchup = 1.03f;      // dsp_loop.rs:790
constexpr float kOwEmergency = 1.06f;       // dsp_loop.rs:791
constexpr float kOwHistoryDecayDb = 0.15f;  // output_writer.rs:226, 281

// The state plane: uint32 [field][n_streams] (floats as their bit patterns).
enum OwField : int {
  kOwEma = 0, kOwFadeRemaining,          // drift_error_ema, discontinuity_fade_remaining
  kOwGain, kOwWriteIdx,                  // TruePeakLimiter::gain_reduction, write_idx (true_peak.rs:254-256)
  kOwSel,                                // which history buffer is current (a push writes the other one)
  // two buffers x (limiter input, limiter output, detector) x 32 frames, newest first: kOwHist + (buffer * 3 + which) * 32 + k.
  // The limiter's 20-frame delay line is the first 20 frames of its input history (both take the same scrubbed frame per
  // step and are reset together), so it has no field of its own.
  kOwHist,
  // the linear statistics of the last push
  kOwInTp = kOwHist + 2 * 3 * kOwTaps, kOwOutTp, kOwDetTp, kOwMinGain, kOwClipMax,
  kOwClipCount, kOwLimited,              // of the push in flight: clipped frames, the limiter's `limited`
  // running counters, low word then high word (output_writer.rs:2-5, 10, 12)
  kOwCntJitterDropped, kOwCntRetimeAdjust = kOwCntJitterDropped + 2, kOwCntRecovery = kOwCntRetimeAdjust + 2,
  kOwCntShortDropped = kOwCntRecovery + 2, kOwCntClip = kOwCntShortDropped + 2, kOwCntTruePeak = kOwCntClip + 2,
  // the dB atomics of output_writer.rs:11-17
  kOwDbClipPeak = kOwCntTruePeak + 2, kOwDbTruePeak, kOwDbTruePeakInput, kOwDbGainReduction, kOwDbGainReductionHistory, kOwDbHeadroom,
  // the decision record of the push in flight: written by the plan pass, read by the passes behind it
  kOwRecRatio, kOwRecOutLen, kOwRecFadeElapsed, kOwRecFadeCount, kOwRecFree, kOwRecWritten, kOwRecSel, kOwRecFillAfter,
  kOwCount
};
enum OwHistory : int { kOwHistIn = 0, kOwHistOut = 1, kOwHistDet = 2 };

// what one push hands every pass
struct OwPush {
  const float *in;         // [n_streams][in_stride]
  int64_t in_stride;
  int32_t n;               // frames per stream, 1..8192
  const int64_t *fill;     // [n_streams]: frames in each stream's queue at the call
  int32_t clean_path;
  float *out;              // [n_streams][out_stride]: row s gets written[s] frames
  int64_t out_stride;
  int64_t *written;        // [n_streams]
  uint32_t *plane;
  int32_t n_streams;
  float *x;                // [n_streams][max_out]: the shaped block, the limiter's input
  float *tg;               // [max_out][n_streams]: the gain each frame asks for, then the gain it gets
  int32_t max_out;         // af_output_writer_max_output_frames(n): no stream's out_len exceeds it
  int32_t limiter_on;
  float ceiling;           // output_ceiling of output_writer.rs:208-212
  float limiter_ceiling;   // ... as TruePeakLimiter::set_ceiling_linear keeps it (true_peak.rs:304-306)
  float clamp_ceiling;     // ... as the final clamp uses it (routing.rs:774)
  float release_coeff;     // TruePeakLimiter::release_coeff at the writer's rate
  int64_t capacity, center, hard, fade;
};

hipError_t launch_output_writer_init(uint32_t *plane, int32_t n_streams, hipStream_t stream);
// pass 1, lane = stream: EMA, ratio, out_len, fade bookkeeping, the modelled queue write and their counters
hipError_t launch_output_writer_plan(const OwPush &p, hipStream_t stream);
// pass 2, lane = output frame: retime gather, fade, scrub; with the limiter on its input-side true peak and target gain
hipError_t launch_output_writer_shape(const OwPush &p, hipStream_t stream);
// pass 3, lane = stream, serial in time: the limiter's gain (only with the limiter on)
hipError_t launch_output_writer_gain(const OwPush &p, hipStream_t stream);
// pass 4, lane = output frame: delayed frame x gain, clamps, the two output-side oversamplers, store, new histories
hipError_t launch_output_writer_out(const OwPush &p, hipStream_t stream);
// pass 5, lane = stream: counters, dB fields, limiter state of a push with the limiter off
hipError_t launch_output_writer_finish(const OwPush &p, hipStream_t stream);

}  // namespace af
