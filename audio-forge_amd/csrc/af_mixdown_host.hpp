// af_mixdown_host.hpp -- what the host side and the kernels of the input mixdown (af_mixdown.hip) share: the constants of
// rust-core/src/audio/input.rs:22-29, the state plane's fields and the launchers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace af {

constexpr int kMixMaxDelay = 8;        // PHASE_SAFE_MAX_DELAY_SAMPLES, input.rs:25
constexpr int kMixLags = 2 * kMixMaxDelay + 1;
constexpr int kMixHistory = 16;        // PHASE_SAFE_HISTORY_SAMPLES, input.rs:28
constexpr int kMixChunk = 8192;        // INPUT_SCRATCH_CAPACITY, input.rs:778: one decision per chunk of a callback
constexpr int kMixMaxChannels = 8;

// InputChannelMode (input.rs:137-144) and PhaseRescueStrategy (input.rs:31-37)
enum MixMode : int { kMixAverage = 0, kMixLeft = 1, kMixRight = 2, kMixMaxRms = 3, kMixPhaseSafeMono = 4 };
enum MixStrategy : int { kMixNone = 0, kMixPolarityFlip = 1, kMixFractionalDelay = 2, kMixMaxRmsFallback = 3 };

// how the mix pass forms a chunk's frames: the decision record's kind
enum MixKind : int {
  kMixKindAverage = 0,    // ((0 + c0) + c1 ...) * (1 / C), input.rs:719-731
  kMixKindSelect = 1,     // one channel, input.rs:681-709 and the max-RMS fallback 561-565
  kMixKindHalfSum = 2,    // 0.5 * (l + r), input.rs:573-577
  kMixKindFlip = 3,       // (l + r * polarity) * gain, input.rs:588-591 (pushes the history)
  kMixKindFractional = 4  // warm-up or the two Lagrange reads, input.rs:593-628 (pushes the history)
};

// The state plane: uint32 [field][n_streams] (floats as their bit patterns).
enum MixField : int {
  kMfHistory = 0,  // two buffers x (left, right) x 16 frames, newest first: field = buffer * 32 + channel * 16 + k
  kMfHistorySel = 4 * kMixHistory,  // which buffer is current (the mix pass of a pushing chunk writes the other one)
  kMfFilled,
  kMfLastValid, kMfLastStrategy, kMfLastDelay, kMfLastPolarity, kMfLastCorrelation,  // PhaseSafeMonoState::last_candidate
  kMfDiagCorrelation, kMfDiagWarnLo, kMfDiagWarnHi, kMfDiagStrategy, kMfDiagDelay, kMfDiagFlipped,  // input.rs:181-186
  // the decision record of the chunk in flight: written by the decision pass, read by the mix pass behind it
  kMfRecKind, kMfRecChannel, kMfRecDelay, kMfRecPolarity, kMfRecGain, kMfRecHistorySel, kMfRecFilled,
  kMfCount
};

// fresh PhaseSafeMonoState and diagnostics (the correlation reads NaN until a first Some)
hipError_t launch_mixdown_init(uint32_t *plane, int32_t n_streams, hipStream_t stream);
// stereo: the decision pass of one chunk.  in: [n_streams][in_stride][2], offset to the chunk's first frame by the caller.
hipError_t launch_mixdown_decide(const float *in, int64_t in_stride, int32_t n, uint32_t *plane, int32_t n_streams, int32_t mode,
                                 hipStream_t stream);
// more than two channels in MaxRms: strongest_channel_index of one chunk, lanes = (stream, channel)
hipError_t launch_mixdown_energy(const float *in, int64_t in_stride, int32_t n, int32_t channels, uint32_t *plane, int32_t n_streams,
                                 hipStream_t stream);
// the mix pass of one chunk.  host_kind < 0: the record the decision / energy pass left; otherwise kMixKindAverage or
// kMixKindSelect with host_channel, decided on the host (no pass in front), and the chunk's diagnostics are "none".
hipError_t launch_mixdown_mix(const float *in, int64_t in_stride, int32_t n, int32_t channels, float *out, int64_t out_stride,
                              uint32_t *plane, int32_t n_streams, int32_t host_kind, int32_t host_channel, hipStream_t stream);

}  // namespace af
