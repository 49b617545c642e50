// af_mixdown.hip -- the input mixdown of the reference's capture callback (rust-core/src/audio/input.rs:383-736, driven per
// callback at :785-843), batched: interleaved device frames -> mono, with the phase-safe stereo rescue.
//
// Every quantity is an IEEE f32 add / mul / div / sqrt in the reference's order (the build is -ffp-contract=off; HIP's f32
// divide and square root are correctly rounded), so the result is bit-exact with a CPU restatement.
//
// Two passes per chunk of at most 8192 frames, in stream order, no host wait between them.
//
// Decision pass (mixdown_decide_kernel).  Each of the 3 x 17 running sums of delayed_correlation (:437-475) has to be
// accumulated in sample order, so the parallelism is streams x lags, not time.  Lane g of a 256-lane workgroup is
// (stream g / 17, lag g % 17 - 8): 15 streams fill 255 lanes.  The workgroup walks the chunk in tiles of 64 frames; all 256
// lanes load a tile (lane = interleaved sample: coalesced), split into a left and a right LDS row per stream with 8 frames
// of halo either side for the lagged reads.  A row is 81 words: with 32 banks for ds_read_b32 and conflicts counted per
// 32-lane half, the right read of lane g sits at word s * 81 + (lag + 8) + t = s * 64 + g + t, i.e. bank (g + t) % 32
// -- 32 consecutive lanes, 32 distinct banks -- and the left read is one broadcast per stream on banks 17 s + c.
// Polarity -1 needs no second walk: l * (-r) == -(l * r) exactly and round-to-nearest is symmetric, so its sum_lr is the
// negation, its sum_r2 the same bits, and its correlation the negated one.  The lag-0 lane's sums are also those of
// stereo_correlation (:409-435) and the two channel energies of strongest_channel_index (:383-407).  One lane per stream
// then gathers the 17 correlations from LDS, runs best_phase_alignment's search (polarity +1 first, lags ascending, strict
// >), the parabola (whose three correlations are among the 17), the hysteresis against last_candidate (:550-558), and
// writes the decision record and the diagnostics into the state plane.  In the other modes stereo still gets its
// correlation and warning count (:833-838): the same kernel with one lag per stream.
//
// Mix pass (mixdown_mix_kernel).  Feed-forward, lane = time.  The history after pushing frame t of the chunk is
// h[k] = x[t - k] for k <= t and the stored history's [k - t - 1] otherwise, and filled = min(filled0 + t + 1, 16), so every
// frame is formed on its own.  A chunk mixed with a candidate stores the new 16-frame history into the other buffer of a
// ping-pong pair (no lane reads what another one writes); the decision pass has already flipped the selector and advanced
// `filled`, as state.push does only on those chunks (:586).
#include "af_mixdown_host.hpp"

#include <cmath>

namespace af {
namespace {

constexpr int kTile = 64;                       // frames per tile of the decision walk
constexpr int kRow = 81;                        // kTile + 2 * 8 halo, padded to == 17 (mod 32)
constexpr int kThreads = 256;
constexpr float kEps = 1.1920929e-07f;          // f32::EPSILON
constexpr float kWarn = -0.75f;                 // INPUT_PHASE_WARNING_CORRELATION, input.rs:24
constexpr float kMinCorr = 0.35f, kMinImprovement = 0.04f;  // input.rs:26-27
constexpr float kLatency = 2.0f;                // PHASE_SAFE_INTERPOLATION_LATENCY, input.rs:29
constexpr float kFrac1Sqrt2 = 0.70710678118654752440f;
static_assert(kRow >= kTile + 2 * kMixMaxDelay && kRow % 32 == kMixLags, "LDS row: halo and bank spread");

__device__ __forceinline__ float clampf(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }  // f32::clamp

struct Plane {
  uint32_t *p;
  int32_t n_streams, s;
  __device__ __forceinline__ uint32_t &u(int f) const { return p[(int64_t)f * n_streams + s]; }
  __device__ __forceinline__ float f(int fld) const { return __uint_as_float(u(fld)); }
  __device__ __forceinline__ void setf(int fld, float v) const { u(fld) = __float_as_uint(v); }
};

__global__ void mixdown_init_kernel(uint32_t *plane, int32_t n_streams) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)kMfCount * n_streams) return;
  plane[i] = (i / n_streams == kMfDiagCorrelation) ? 0x7fc00000u : 0u;
}

// strongest_channel_index over energies already summed (input.rs:392-406): first maximum wins, from -inf
__device__ __forceinline__ int strongest2(float e0, float e1) {
  int best = 0;
  float be = -INFINITY;
  if (e0 > be) be = e0;
  if (e1 > be) best = 1;
  return best;
}

// What one stream's lane does once the sums are in: the callback's diagnostics (:825-838) and the decision record.
// corr / valid: the 17 delayed correlations at polarity +1 (nullptr outside the phase-safe mode).
__device__ void decide_stream(const Plane st, int mode, int n, bool sc_valid, float sc, float e0, float e1, const float *corr,
                              const int *valid) {
  if (sc_valid) {
    st.setf(kMfDiagCorrelation, sc);
    if (sc < kWarn) {
      const uint32_t lo = st.u(kMfDiagWarnLo) + 1u;
      st.u(kMfDiagWarnLo) = lo;
      if (lo == 0u) st.u(kMfDiagWarnHi) += 1u;
    }
  }
  int kind = kMixKindAverage, channel = 0, strategy = kMixNone, flipped = 0;
  float delay = 0.0f, polarity = 1.0f, gain = 1.0f, d_delay = 0.0f;
  if (mode == kMixLeft) {
    kind = kMixKindSelect;
  } else if (mode == kMixRight) {
    kind = kMixKindSelect;
    channel = 1;
  } else if (mode == kMixMaxRms) {
    kind = kMixKindSelect;
    channel = strongest2(e0, e1);
  } else if (mode == kMixPhaseSafeMono) {
    const float current = sc_valid ? sc : 1.0f;
    // best_phase_alignment, :486-502
    int best_delay = 0;
    float best_polarity = 1.0f, best_corr = -INFINITY;
    for (int i = 0; i < kMixLags; ++i)
      if (valid[i] && corr[i] > best_corr) {
        best_corr = corr[i];
        best_delay = i - kMixMaxDelay;
      }
    for (int i = 0; i < kMixLags; ++i)
      if (valid[i] && -corr[i] > best_corr) {
        best_corr = -corr[i];
        best_delay = i - kMixMaxDelay;
        best_polarity = -1.0f;
      }
    bool c_valid = false;
    int c_strategy = kMixNone;
    float c_delay = 0.0f, c_polarity = 0.0f, c_corr = 0.0f;
    if (!(best_corr < kMinCorr || best_corr - current < kMinImprovement)) {  // :504-508
      float refined = (float)best_delay;
      if (best_delay > -kMixMaxDelay && best_delay < kMixMaxDelay) {
        const int i = best_delay + kMixMaxDelay;
        if (valid[i - 1] && valid[i] && valid[i + 1]) {
          const float prev = corr[i - 1] * best_polarity, center = corr[i] * best_polarity, next = corr[i + 1] * best_polarity;
          const float denom = prev - 2.0f * center + next;
          if (fabsf(denom) > 1e-6f) refined += clampf(0.5f * (prev - next) / denom, -0.5f, 0.5f);
        }
      }
      c_valid = true;
      c_strategy = (best_polarity < 0.0f && fabsf(refined) < 0.25f) ? kMixPolarityFlip : kMixFractionalDelay;
      c_delay = refined;
      c_polarity = best_polarity;
      c_corr = best_corr;
    }
    // the hysteresis, :553-558
    if (c_valid) {
      st.u(kMfLastValid) = 1u;
      st.u(kMfLastStrategy) = (uint32_t)c_strategy;
      st.setf(kMfLastDelay, c_delay);
      st.setf(kMfLastPolarity, c_polarity);
      st.setf(kMfLastCorrelation, c_corr);
    } else if (current >= kWarn) {
      st.u(kMfLastValid) = 0u;
    } else if (st.u(kMfLastValid)) {
      c_valid = true;
      c_strategy = (int)st.u(kMfLastStrategy);
      c_delay = st.f(kMfLastDelay);
      c_polarity = st.f(kMfLastPolarity);
      c_corr = st.f(kMfLastCorrelation);
    }
    if (!c_valid) {
      if (current < kWarn) {  // :560-570
        kind = kMixKindSelect;
        channel = strongest2(e0, e1);
        strategy = kMixMaxRmsFallback;
      } else {
        kind = kMixKindHalfSum;
      }
    } else {
      const float c0 = c_corr > 0.0f ? c_corr : 0.0f;
      gain = clampf(1.0f / (2.0f * sqrtf(0.5f + 0.5f * c0)), 0.5f, kFrac1Sqrt2);  // :581-582
      kind = c_strategy == kMixPolarityFlip ? kMixKindFlip : kMixKindFractional;
      delay = c_delay;
      polarity = c_polarity;
      strategy = c_strategy;
      d_delay = c_delay;
      flipped = c_polarity < 0.0f;
      // state.push runs on every frame of such a chunk: the mix pass writes the other history buffer
      const uint32_t sel = st.u(kMfHistorySel), filled = st.u(kMfFilled);
      st.u(kMfRecHistorySel) = sel;
      st.u(kMfRecFilled) = filled;
      st.u(kMfHistorySel) = sel ^ 1u;
      st.u(kMfFilled) = filled + (uint32_t)n < (uint32_t)kMixHistory ? filled + (uint32_t)n : (uint32_t)kMixHistory;
    }
  }
  st.u(kMfRecKind) = (uint32_t)kind;
  st.u(kMfRecChannel) = (uint32_t)channel;
  st.setf(kMfRecDelay, delay);
  st.setf(kMfRecPolarity, polarity);
  st.setf(kMfRecGain, gain);
  st.u(kMfDiagStrategy) = (uint32_t)strategy;
  st.setf(kMfDiagDelay, d_delay);
  st.u(kMfDiagFlipped) = (uint32_t)flipped;
}

// NL = 17: phase-safe mode, lanes = (stream, lag), 15 streams per workgroup.  NL = 1: the other modes, lag 0 only.
template <int NL>
__global__ __launch_bounds__(kThreads) void mixdown_decide_kernel(const float *__restrict__ in, int64_t in_stride, int32_t n,
                                                                  uint32_t *plane, int32_t n_streams, int32_t mode) {
  constexpr int SPB = NL == kMixLags ? kThreads / kMixLags : 32;
  __shared__ float s_left[SPB * kRow], s_right[SPB * kRow];
  __shared__ float s_corr[SPB][kMixLags];
  __shared__ int s_valid[SPB][kMixLags];
  __shared__ float s_stereo[SPB][4];  // stereo correlation, its validity, energy of left, of right
  const int tid = threadIdx.x;
  const int s0 = blockIdx.x * SPB;
  const int ls = tid / NL, li = tid - ls * NL;
  const int lag = NL == kMixLags ? li - kMixMaxDelay : 0;
  const bool walker = ls < SPB && s0 + ls < n_streams;
  const int start = lag < 0 ? -lag : 0;                       // :447-452
  const int end = lag > 0 ? (n > lag ? n - lag : 0) : n;
  float sum_lr = 0.0f, sum_l2 = 0.0f, sum_r2 = 0.0f;

  for (int t0 = 0; t0 < n; t0 += kTile) {
    // load role: lane = interleaved sample of [t0 - 8, t0 + 72) of each stream; outside the chunk: zeros (never summed)
    constexpr int kSpan = kTile + 2 * kMixMaxDelay;
    for (int i = tid; i < SPB * kSpan * 2; i += kThreads) {
      const int sl = i / (kSpan * 2), j = i - sl * (kSpan * 2);
      const int fr = j >> 1, ch = j & 1, t = t0 - kMixMaxDelay + fr, s = s0 + sl;
      float v = 0.0f;
      if (s < n_streams && t >= 0 && t < n) v = in[((int64_t)s * in_stride + t) * 2 + ch];
      (ch ? s_right : s_left)[sl * kRow + fr] = v;
    }
    __syncthreads();
    if (walker) {
      const int lo = start > t0 ? start : t0, hi = end < t0 + kTile ? end : t0 + kTile;
      const float *pl = s_left + ls * kRow + kMixMaxDelay - t0;         // pl[t]: left frame t
      const float *pr = s_right + ls * kRow + kMixMaxDelay - t0 + lag;  // pr[t]: right frame t + lag (within the halo)
#pragma unroll 8
      for (int t = lo; t < hi; ++t) {  // :460-467, in sample order
        const float l = pl[t], r = pr[t];
        sum_lr += l * r;
        sum_l2 += l * l;
        sum_r2 += r * r;
      }
    }
    __syncthreads();
  }

  if (walker) {
    const float denom = sqrtf(sum_l2 * sum_r2);  // :469-474
    const bool some = !(denom <= kEps);
    const float c = clampf(sum_lr / denom, -1.0f, 1.0f);
    s_corr[ls][li] = c;
    s_valid[ls][li] = (end > start && end - start >= 3 && some) ? 1 : 0;  // :453
    if (lag == 0) {  // stereo_correlation: the same sums over [0, n), no 3-frame rule (:414, :429-434)
      s_stereo[ls][0] = c;
      s_stereo[ls][1] = (n > 0 && some) ? 1.0f : 0.0f;
      s_stereo[ls][2] = sum_l2;
      s_stereo[ls][3] = sum_r2;
    }
  }
  __syncthreads();
  if (tid < SPB && s0 + tid < n_streams) {
    const Plane st{plane, n_streams, s0 + tid};
    decide_stream(st, mode, n, s_stereo[tid][1] != 0.0f, s_stereo[tid][0], s_stereo[tid][2], s_stereo[tid][3],
                  NL == kMixLags ? s_corr[tid] : nullptr, NL == kMixLags ? s_valid[tid] : nullptr);
  }
}

// channels != 2, MaxRms: lanes = (stream, channel), each its own energy in sample order; one lane per stream picks
__global__ __launch_bounds__(kThreads) void mixdown_energy_kernel(const float *__restrict__ in, int64_t in_stride, int32_t n,
                                                                  int32_t channels, uint32_t *plane, int32_t n_streams) {
  __shared__ float s_energy[kThreads];
  const int tid = threadIdx.x;
  const int spb = kThreads / channels;
  const int ls = tid / channels, c = tid - ls * channels;
  const int s = blockIdx.x * spb + ls;
  const bool active = ls < spb && s < n_streams;
  float energy = 0.0f;
  if (active) {
    const float *x = in + (int64_t)s * in_stride * channels + c;
    for (int t = 0; t < n; ++t) {
      const float v = x[(int64_t)t * channels];
      energy += v * v;
    }
  }
  s_energy[tid] = energy;
  __syncthreads();
  if (active && c == 0) {
    int best = 0;
    float be = -INFINITY;
    for (int k = 0; k < channels; ++k)
      if (s_energy[tid + k] > be) {
        be = s_energy[tid + k];
        best = k;
      }
    const Plane st{plane, n_streams, s};
    st.u(kMfRecKind) = (uint32_t)kMixKindSelect;
    st.u(kMfRecChannel) = (uint32_t)best;
    st.u(kMfDiagStrategy) = (uint32_t)kMixNone;
    st.setf(kMfDiagDelay, 0.0f);
    st.u(kMfDiagFlipped) = 0u;
  }
}

// PhaseSafeMonoState::lagrange_sample (:121-134) on the history as it stands after pushing frame t
struct Taps {
  const float *x;        // the chunk's frames of this stream, interleaved stereo
  const uint32_t *old;   // plane field of the stored history's [0] of this channel, for this stream
  int64_t field_stride;  // n_streams
  int t, ch;
  __device__ __forceinline__ float at(int k) const {
    const int idx = t - k;
    return idx >= 0 ? x[(int64_t)idx * 2 + ch] : __uint_as_float(old[(int64_t)(k - t - 1) * field_stride]);
  }
};

__device__ __forceinline__ float lagrange_sample(const Taps h, float delay) {
  delay = clampf(delay, 2.0f, (float)(kMixHistory - 3));
  const int upper = (int)ceilf(delay);
  const float t = (float)upper - delay;
  const float x0 = h.at(upper + 1), x1 = h.at(upper), x2 = h.at(upper - 1), x3 = h.at(upper - 2);
  const float l0 = -t * (t - 1.0f) * (t - 2.0f) / 6.0f;
  const float l1 = (t + 1.0f) * (t - 1.0f) * (t - 2.0f) / 2.0f;
  const float l2 = -(t + 1.0f) * t * (t - 2.0f) / 2.0f;
  const float l3 = (t + 1.0f) * t * (t - 1.0f) / 6.0f;
  return x0 * l0 + x1 * l1 + x2 * l2 + x3 * l3;
}

__global__ __launch_bounds__(kThreads) void mixdown_mix_kernel(const float *__restrict__ in, int64_t in_stride, int32_t n,
                                                               int32_t channels, float *__restrict__ out, int64_t out_stride,
                                                               uint32_t *plane, int32_t n_streams, int32_t host_kind,
                                                               int32_t host_channel) {
  const int blocks_per_stream = (n + kThreads - 1) / kThreads;
  const int s = blockIdx.x / blocks_per_stream, block = blockIdx.x - s * blocks_per_stream;
  const int t = block * kThreads + threadIdx.x;
  const Plane st{plane, n_streams, s};
  const int kind = host_kind >= 0 ? host_kind : (int)st.u(kMfRecKind);
  const float *x = in + (int64_t)s * in_stride * channels;

  if (host_kind >= 0 && block == 0 && threadIdx.x == 0) {  // no pass in front: the chunk's diagnostics are "none"
    st.u(kMfDiagStrategy) = (uint32_t)kMixNone;
    st.setf(kMfDiagDelay, 0.0f);
    st.u(kMfDiagFlipped) = 0u;
  }
  const bool pushes = kind == kMixKindFlip || kind == kMixKindFractional;  // (stereo only: the decision pass's kinds)
  const int sel = pushes ? (int)st.u(kMfRecHistorySel) : 0;
  if (pushes && block == 0 && threadIdx.x < 2 * kMixHistory) {  // the history after the chunk, into the other buffer
    const int ch = threadIdx.x >> 4, k = threadIdx.x & 15;
    const float v = k < n ? x[(int64_t)(n - 1 - k) * 2 + ch] : st.f(kMfHistory + sel * 32 + ch * 16 + (k - n));
    st.setf(kMfHistory + (sel ^ 1) * 32 + ch * 16 + k, v);
  }
  if (t >= n) return;

  float y;
  if (kind == kMixKindAverage) {
    const float inv = 1.0f / (float)channels;
    float sum = 0.0f;
    for (int c = 0; c < channels; ++c) sum += x[(int64_t)t * channels + c];
    y = sum * inv;
  } else if (kind == kMixKindSelect) {
    const int ch = host_kind >= 0 ? host_channel : (int)st.u(kMfRecChannel);
    y = x[(int64_t)t * channels + ch];
  } else {
    const float l = x[(int64_t)t * 2], r = x[(int64_t)t * 2 + 1];
    if (kind == kMixKindHalfSum) {
      y = 0.5f * (l + r);
    } else {
      const float polarity = st.f(kMfRecPolarity), gain = st.f(kMfRecGain);
      if (kind == kMixKindFlip) {
        y = (l + r * polarity) * gain;
      } else {
        const float delay = st.f(kMfRecDelay);
        const int required = (int)ceilf(kLatency + fabsf(delay)) + 2;  // :593-595
        const int filled0 = (int)st.u(kMfRecFilled);
        const int filled = filled0 + t + 1 < kMixHistory ? filled0 + t + 1 : kMixHistory;
        if (filled <= required) {
          y = fabsf(l) >= fabsf(r) ? l : r;  // :596-602
        } else {
          const uint32_t *old = plane + (int64_t)(kMfHistory + sel * 32) * n_streams + s;
          const Taps hl{x, old, n_streams, t, 0}, hr{x, old + (int64_t)16 * n_streams, n_streams, t, 1};
          float al, ar;
          if (delay >= 0.0f) {  // :605-627
            al = lagrange_sample(hl, kLatency + delay);
            ar = lagrange_sample(hr, kLatency);
          } else {
            al = lagrange_sample(hl, kLatency);
            ar = lagrange_sample(hr, kLatency - delay);
          }
          y = (al + ar * polarity) * gain;
        }
      }
    }
  }
  out[(int64_t)s * out_stride + t] = y;
}

}  // namespace

hipError_t launch_mixdown_init(uint32_t *plane, int32_t n_streams, hipStream_t stream) {
  const int64_t total = (int64_t)kMfCount * n_streams;
  hipLaunchKernelGGL(mixdown_init_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, plane, n_streams);
  return hipGetLastError();
}

hipError_t launch_mixdown_decide(const float *in, int64_t in_stride, int32_t n, uint32_t *plane, int32_t n_streams, int32_t mode,
                                 hipStream_t stream) {
  if (mode == kMixPhaseSafeMono) {
    constexpr int spb = kThreads / kMixLags;
    hipLaunchKernelGGL(mixdown_decide_kernel<kMixLags>, dim3((unsigned)((n_streams + spb - 1) / spb)), dim3(kThreads), 0, stream, in,
                       in_stride, n, plane, n_streams, mode);
  } else {
    hipLaunchKernelGGL(mixdown_decide_kernel<1>, dim3((unsigned)((n_streams + 31) / 32)), dim3(kThreads), 0, stream, in, in_stride, n,
                       plane, n_streams, mode);
  }
  return hipGetLastError();
}

hipError_t launch_mixdown_energy(const float *in, int64_t in_stride, int32_t n, int32_t channels, uint32_t *plane, int32_t n_streams,
                                 hipStream_t stream) {
  const int spb = kThreads / channels;
  hipLaunchKernelGGL(mixdown_energy_kernel, dim3((unsigned)((n_streams + spb - 1) / spb)), dim3(kThreads), 0, stream, in, in_stride, n,
                     channels, plane, n_streams);
  return hipGetLastError();
}

hipError_t launch_mixdown_mix(const float *in, int64_t in_stride, int32_t n, int32_t channels, float *out, int64_t out_stride,
                              uint32_t *plane, int32_t n_streams, int32_t host_kind, int32_t host_channel, hipStream_t stream) {
  hipLaunchKernelGGL(mixdown_mix_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads) * (unsigned)n_streams), dim3(kThreads), 0, stream,
                     in, in_stride, n, channels, out, out_stride, plane, n_streams, host_kind, host_channel);
  return hipGetLastError();
}

}  // namespace af
