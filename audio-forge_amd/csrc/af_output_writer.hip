// af_output_writer.hip -- the reference's output writer (rust-core/src/audio/processor/output_writer.rs:62-343), batched:
// what every block goes through between the chain / output resampler and the playback queue.  Drift retime
// (:112-159 over resampling.rs:81-120), discontinuity fade (:161-192), safety (:194-288: scrub, a second TruePeakLimiter,
// ceiling clamp with clip metrics, a TruePeakDetector) and the queue write's accounting (:290-343) against a queue whose
// fill the caller reports.
//
// Every quantity is an IEEE f32 operation in the reference's order (the build is -ffp-contract=off; HIP's f32 divide is
// correctly rounded; the only FMAs are the explicit ones of the true-peak FIR), so audio, decisions, counters and linear
// statistics are bit-exact with a CPU restatement.  The dB fields go through the device's log10f.
//
// Five passes per push, in stream order, no host wait between them.  The output is ragged: stream s has out_len[s]
// frames, known only on the device, so the frame-parallel passes launch for the longest possible block and a workgroup
// whose tile starts past its stream's out_len leaves at once.
//
//   plan   lane = stream.  EMA, ratio, out_len, the fade window, free / written, their counters: the decision record.
//   shape  lane = output frame, 256 frames of one stream per workgroup.  The two-tap gather, the fade factor, the scrub;
//          the tile and the 31 frames before it (from the stored history before the block's first frame) go through LDS
//          for the limiter's input-side 4 x 32-tap peak, which becomes the gain the frame asks for (the division of
//          true_peak.rs:350-354 happens here, in parallel).  Target gains are stored time-major, [frame][stream].
//   gain   lane = stream, serial over out_len[s]: true_peak.rs:355-361, two multiplies and an add per frame, reads and
//          writes coalesced across streams.  The gain overwrites the target in place.
//   out    lane = output frame.  Delayed frame x gain, limiter clamp, ceiling clamp with the clip metrics, the limiter's
//          output oversampler and the detector's (their histories differ after a limiter reset), per-stream maxima by wave
//          reduction and one atomic per wave on the bit patterns (non-negative floats order as unsigned integers), the first
//          written[s] frames to the caller's row, the new histories from the full out_len frames into the other buffer of
//          a ping-pong pair (no lane reads what another one writes).
//   finish lane = stream.  64-bit counters, dB fields, the limiter's state after a push with the limiter off.
#include "af_output_writer_host.hpp"

#include <cmath>

#include "tp_fir_table.h"

namespace af {
namespace {

constexpr int kThreads = 256;
constexpr int kHalo = kOwTaps - 1;

__device__ __forceinline__ float clampf(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }  // f32::clamp
__device__ __forceinline__ bool finite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

struct Plane {
  uint32_t *p;
  int32_t n_streams, s;
  __device__ __forceinline__ uint32_t &u(int f) const { return p[(int64_t)f * n_streams + s]; }
  __device__ __forceinline__ float f(int fld) const { return __uint_as_float(u(fld)); }
  __device__ __forceinline__ void setf(int fld, float v) const { u(fld) = __float_as_uint(v); }
  __device__ __forceinline__ int hist(int sel, int which, int k) const { return kOwHist + (sel * 3 + which) * kOwTaps + k; }
  __device__ __forceinline__ void add64(int fld, uint64_t v) const {
    const uint64_t cur = ((uint64_t)u(fld) | ((uint64_t)u(fld + 1) << 32)) + v;
    u(fld) = (uint32_t)cur;
    u(fld + 1) = (uint32_t)(cur >> 32);
  }
};

// Bandlimited4xPeak::observe (true_peak.rs:173-186) of the frame at w[i]: w[i - k] is the frame k steps back
__device__ __forceinline__ float tp_observe_lds(const float *w, int i) {
  float peak = fabsf(w[i]);
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < kOwTaps; ++k) acc = __builtin_fmaf(AF_TP_FIR[p][k], w[i - k], acc);
    peak = fmaxf(peak, fabsf(acc));
  }
  return peak;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ void ow_init_kernel(uint32_t *plane, int32_t n_streams) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)kOwCount * n_streams) return;
  // dsp_loop.rs:796-802 and the atomics' initial values, processor.rs:659-668
  float v = 0.0f;
  switch ((int)(i / n_streams)) {
    case kOwGain: case kOwMinGain: case kOwRecRatio: v = 1.0f; break;
    case kOwDbClipPeak: case kOwDbTruePeak: case kOwDbTruePeakInput: v = -120.0f; break;
    case kOwDbHeadroom: v = 120.0f; break;
    default: break;
  }
  plane[i] = __float_as_uint(v);
}

// ---- pass 1 (output_writer.rs:67-69, 112-159, 168-190, 298-309, 333-343)
__global__ void ow_plan_kernel(OwPush a) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= a.n_streams) return;
  const Plane P{a.plane, a.n_streams, s};
  const int64_t n = a.n;
  int64_t fill = a.fill[s];
  fill = fill < 0 ? 0 : (fill > a.capacity ? a.capacity : fill);  // (the host entry point refuses such a call)
  const int64_t free_len = a.capacity - fill;
  int64_t out_len = n, fade_count = 0, fade_elapsed = 0;
  float ratio = 1.0f;
  if (!a.clean_path) {
    const float error = (float)fill - (float)a.center;
    const float ema = P.f(kOwEma) * 0.85f + error * 0.15f;
    P.setf(kOwEma, ema);
    const int64_t pz = a.hard > a.center ? a.hard - a.center : 0;
    const float positive_zone = (float)(pz < 1 ? 1 : pz), negative_zone = (float)(a.center < 1 ? 1 : a.center);
    const float normalized = ema >= 0.0f ? clampf(ema / positive_zone, 0.0f, 1.0f) : clampf(ema / negative_zone, -1.0f, 0.0f);
    ratio = clampf(1.0f + normalized * kOwRatioAdjust, kOwMinRatio, kOwMaxCatchup);
    if (fill >= a.hard) ratio = kOwEmergency;
    // retime_audio_block's length, resampling.rs:92-94
    const float clamped_ratio = fmaxf(ratio, 0.5f);
    const int64_t desired = (int64_t)fmaxf(roundf((float)n / clamped_ratio), 1.0f);
    const int64_t cap1 = a.capacity < 1 ? 1 : a.capacity;
    out_len = desired < cap1 ? desired : cap1;
    if (out_len > kOwScratch) out_len = kOwScratch;
    if (out_len > a.max_out) out_len = a.max_out;  // (never: max_out is the bound of this expression over every ratio)
    if (out_len != n) {
      if (out_len < n) P.add64(kOwCntJitterDropped, (uint64_t)(n - out_len));
      P.add64(kOwCntRetimeAdjust, 1);
    }
    const int64_t fade_remaining = P.u(kOwFadeRemaining);
    if (fade_remaining != 0) {
      fade_count = fade_remaining < out_len ? fade_remaining : out_len;
      fade_elapsed = a.fade > fade_remaining ? a.fade - fade_remaining : 0;
      P.u(kOwFadeRemaining) = (uint32_t)(fade_remaining - fade_count);
    }
  }
  int64_t written = out_len;
  if (out_len > free_len) {
    P.add64(kOwCntShortDropped, (uint64_t)(out_len - free_len));
    P.add64(kOwCntRecovery, 1);
    P.u(kOwFadeRemaining) = (uint32_t)a.fade;
    written = free_len;
  }
  a.written[s] = written;
  const uint32_t sel = P.u(kOwSel) & 1u;
  P.u(kOwRecSel) = sel;  // the passes behind read buffer `sel` and write the other one, which is current from here on
  P.u(kOwSel) = sel ^ 1u;
  P.setf(kOwRecRatio, ratio);
  P.u(kOwRecOutLen) = (uint32_t)out_len;
  P.u(kOwRecFadeElapsed) = (uint32_t)fade_elapsed;
  P.u(kOwRecFadeCount) = (uint32_t)fade_count;
  P.u(kOwRecFree) = (uint32_t)free_len;
  P.u(kOwRecWritten) = (uint32_t)written;
  P.u(kOwRecFillAfter) = (uint32_t)(fill + written);
  // the accumulators of the passes behind
  P.u(kOwInTp) = 0u;
  P.u(kOwOutTp) = 0u;
  P.u(kOwDetTp) = 0u;
  P.u(kOwClipMax) = 0u;
  P.u(kOwClipCount) = 0u;
  P.u(kOwLimited) = 0u;
}

// ---- pass 2
__global__ __launch_bounds__(kThreads) void ow_shape_kernel(OwPush a) {
  __shared__ float xs[kThreads + kHalo];
  const int s = blockIdx.y;
  const Plane P{a.plane, a.n_streams, s};
  const int out_len = (int)P.u(kOwRecOutLen);
  const int t0 = blockIdx.x * kThreads;
  if (t0 >= out_len) return;
  const int n = a.n;
  const bool gather = !a.clean_path && out_len != n;  // resampling.rs:95-97: a block of the same length passes through
  const float ratio = fmaxf(P.f(kOwRecRatio), 0.5f);
  const int fade_count = (int)P.u(kOwRecFadeCount), fade_elapsed = (int)P.u(kOwRecFadeElapsed);
  const float fade_total = (float)a.fade;
  const int sel = (int)P.u(kOwRecSel);
  const float *in = a.in + (int64_t)s * a.in_stride;
  const float max_src = (float)(n - 1);
  for (int j = threadIdx.x; j < kThreads + kHalo; j += kThreads) {
    const int t = t0 - kHalo + j;
    float v = 0.0f;
    if (t < 0) {
      if (a.limiter_on) v = P.f(P.hist(sel, kOwHistIn, -1 - t));
    } else if (t < out_len) {
      if (gather) {  // resampling.rs:104-117
        const float src_pos = out_len == 1 ? 0.0f : fminf((float)t * ratio, max_src);
        const int idx0 = (int)floorf(src_pos);
        const int idx1 = idx0 + 1 < n - 1 ? idx0 + 1 : n - 1;
        const float frac = src_pos - (float)idx0;
        const float y0 = in[idx0], y1 = in[idx1];
        v = y0 + (y1 - y0) * frac;
      } else {
        v = in[t];
      }
      if (t < fade_count) v *= clampf((float)(fade_elapsed + t + 1) / fade_total, 0.0f, 1.0f);  // output_writer.rs:187-188
      if (!finite_bits(v)) v = 0.0f;  // routing.rs:697-703
    }
    xs[j] = v;
  }
  __syncthreads();
  const int t = t0 + threadIdx.x;
  const bool valid = t < out_len;
  if (valid) a.x[(int64_t)s * a.max_out + t] = xs[threadIdx.x + kHalo];
  if (!a.limiter_on) return;
  float peak = 0.0f;
  if (valid) {
    peak = tp_observe_lds(xs, threadIdx.x + kHalo);
    float target = 1.0f;  // true_peak.rs:350-354
    if (peak > a.limiter_ceiling) target = clampf((a.limiter_ceiling * 0.999f) / peak, 0.0f, 1.0f);
    a.tg[(int64_t)t * a.n_streams + s] = target;
  }
  peak = wave_max(peak);
  if ((threadIdx.x & 63) == 0) atomicMax(&P.u(kOwInTp), __float_as_uint(peak));
}

// ---- pass 3 (true_peak.rs:355-361)
__global__ __launch_bounds__(64) void ow_gain_kernel(OwPush a) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= a.n_streams) return;
  const Plane P{a.plane, a.n_streams, s};
  const int n = (int)P.u(kOwRecOutLen);
  const float rel = a.release_coeff, one_m_rel = 1.0f - a.release_coeff;
  float g = P.f(kOwGain), gmin = INFINITY;
  bool limited = false;
  float *col = a.tg + s;
  const int64_t B = a.n_streams;
  constexpr int kU = 8;
  int t = 0;
  for (; t + kU <= n; t += kU) {
    float v[kU];
#pragma unroll
    for (int k = 0; k < kU; ++k) v[k] = col[(int64_t)(t + k) * B];
#pragma unroll
    for (int k = 0; k < kU; ++k) {
      if (v[k] < g) {
        g = v[k];
        limited = true;
      } else {
        g = rel * g + one_m_rel * v[k];
      }
      gmin = fminf(gmin, g);
      v[k] = g;
    }
#pragma unroll
    for (int k = 0; k < kU; ++k) col[(int64_t)(t + k) * B] = v[k];
  }
  for (; t < n; ++t) {
    const float target = col[(int64_t)t * B];
    if (target < g) {
      g = target;
      limited = true;
    } else {
      g = rel * g + one_m_rel * target;
    }
    gmin = fminf(gmin, g);
    col[(int64_t)t * B] = g;
  }
  P.setf(kOwGain, g);
  P.setf(kOwMinGain, gmin);
  P.u(kOwLimited) = limited ? 1u : 0u;
}

// ---- pass 4
__global__ __launch_bounds__(kThreads) void ow_out_kernel(OwPush a) {
  __shared__ float ys[kThreads + kHalo], zs[kThreads + kHalo];
  const int s = blockIdx.y;
  const Plane P{a.plane, a.n_streams, s};
  const int out_len = (int)P.u(kOwRecOutLen);
  const int t0 = blockIdx.x * kThreads;
  if (t0 >= out_len) return;
  const int written = (int)P.u(kOwRecWritten);
  const int sel = (int)P.u(kOwRecSel), nsel = sel ^ 1;
  const float *x = a.x + (int64_t)s * a.max_out;
  const float lc = a.limiter_ceiling, fc = a.clamp_ceiling;
  for (int j = threadIdx.x; j < kThreads + kHalo; j += kThreads) {
    const int t = t0 - kHalo + j;
    float y = 0.0f, z = 0.0f;
    if (t < 0) {
      if (a.limiter_on) y = P.f(P.hist(sel, kOwHistOut, -1 - t));
      z = P.f(P.hist(sel, kOwHistDet, -1 - t));
    } else if (t < out_len) {
      if (a.limiter_on) {  // true_peak.rs:343, 367-369
        const float delayed = t >= kOwLookahead ? x[t - kOwLookahead] : P.f(P.hist(sel, kOwHistIn, kOwLookahead - 1 - t));
        y = clampf(delayed * a.tg[(int64_t)t * a.n_streams + s], -lc, lc);
        if (!finite_bits(y)) y = 0.0f;
      } else {
        y = x[t];
      }
      z = clampf(y, -fc, fc);  // routing.rs:788 (y is finite)
    }
    ys[j] = y;
    zs[j] = z;
  }
  __syncthreads();
  const int t = t0 + threadIdx.x, i = threadIdx.x + kHalo;
  const bool valid = t < out_len;
  float out_tp = 0.0f, det_tp = 0.0f, clip_max = 0.0f;
  bool clipped = false;
  if (valid) {
    const float y = ys[i], z = zs[i];
    const float amplitude = fabsf(y);  // routing.rs:783-787
    clipped = amplitude > fc;
    if (clipped) clip_max = amplitude;
    if (a.limiter_on) out_tp = tp_observe_lds(ys, i);
    det_tp = tp_observe_lds(zs, i);
    if (t < written) a.out[(int64_t)s * a.out_stride + t] = z;
    const int k = out_len - 1 - t;  // frame t is k steps back from the block's end
    if (k < kOwTaps) {
      P.setf(P.hist(nsel, kOwHistDet, k), z);
      if (a.limiter_on) {
        P.setf(P.hist(nsel, kOwHistOut, k), y);
        P.setf(P.hist(nsel, kOwHistIn, k), x[t]);
      }
    }
  }
  if (t0 == 0 && threadIdx.x < kOwTaps) {  // what a block shorter than a history leaves of the old one; a reset limiter's zeros
    const int k = threadIdx.x;
    if (k >= out_len) P.u(P.hist(nsel, kOwHistDet, k)) = P.u(P.hist(sel, kOwHistDet, k - out_len));
    if (!a.limiter_on) {
      P.u(P.hist(nsel, kOwHistIn, k)) = 0u;
      P.u(P.hist(nsel, kOwHistOut, k)) = 0u;
    } else if (k >= out_len) {
      P.u(P.hist(nsel, kOwHistIn, k)) = P.u(P.hist(sel, kOwHistIn, k - out_len));
      P.u(P.hist(nsel, kOwHistOut, k)) = P.u(P.hist(sel, kOwHistOut, k - out_len));
    }
  }
  out_tp = wave_max(out_tp);
  det_tp = wave_max(det_tp);
  clip_max = wave_max(clip_max);
  const uint32_t n_clipped = (uint32_t)__popcll(__ballot(clipped));
  if ((threadIdx.x & 63) == 0) {
    if (a.limiter_on) atomicMax(&P.u(kOwOutTp), __float_as_uint(out_tp));
    atomicMax(&P.u(kOwDetTp), __float_as_uint(det_tp));
    if (n_clipped) {
      atomicMax(&P.u(kOwClipMax), __float_as_uint(clip_max));
      atomicAdd(&P.u(kOwClipCount), n_clipped);
    }
  }
}

// ---- pass 5 (output_writer.rs:214-228, 244-288; routing.rs:651-655, 791-798)
__device__ __forceinline__ void decaying_peak_db(const Plane &P, float value_db) {
  const float previous = fmaxf(P.f(kOwDbGainReductionHistory), 0.0f);
  const float decayed = fmaxf(previous - fmaxf(kOwHistoryDecayDb, 0.0f), 0.0f);
  P.setf(kOwDbGainReductionHistory, fmaxf(value_db, decayed));
}

__global__ void ow_finish_kernel(OwPush a) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= a.n_streams) return;
  const Plane P{a.plane, a.n_streams, s};
  if (a.limiter_on) {
    if (P.u(kOwLimited)) P.add64(kOwCntTruePeak, 1);
    P.setf(kOwDbTruePeakInput, 20.0f * log10f(fmaxf(P.f(kOwInTp), 1e-10f)));
    // the largest current_gain_reduction_db of the block (true_peak.rs:315-321, 363-365) is that of its smallest gain
    const float gmin = P.f(kOwMinGain);
    const float reduction_db = gmin >= 1.0f ? 0.0f : -20.0f * log10f(fmaxf(gmin, 1e-10f));
    P.setf(kOwDbGainReduction, reduction_db);
    decaying_peak_db(P, reduction_db);
    P.u(kOwWriteIdx) = (P.u(kOwWriteIdx) + P.u(kOwRecOutLen)) % kOwLookahead;
  } else {  // TruePeakLimiter::reset, true_peak.rs:289-298 (the out pass zeroed its two histories)
    P.setf(kOwGain, 1.0f);
    P.u(kOwWriteIdx) = 0u;
    P.setf(kOwMinGain, 1.0f);
    P.setf(kOwDbGainReduction, 0.0f);
    decaying_peak_db(P, 0.0f);
  }
  const uint32_t n_clipped = P.u(kOwClipCount);
  if (n_clipped) {
    P.add64(kOwCntClip, n_clipped);
    const float peak_db = 20.0f * log10f(P.f(kOwClipMax));
    if (peak_db > P.f(kOwDbClipPeak)) P.setf(kOwDbClipPeak, peak_db);
  }
  const float true_peak = P.f(kOwDetTp);
  P.setf(kOwDbTruePeak, 20.0f * log10f(fmaxf(true_peak, 1e-10f)));
  P.setf(kOwDbHeadroom, 20.0f * log10f(fmaxf(a.ceiling, 1e-10f) / fmaxf(true_peak, 1e-10f)));
}

}  // namespace

hipError_t launch_output_writer_init(uint32_t *plane, int32_t n_streams, hipStream_t stream) {
  const int64_t total = (int64_t)kOwCount * n_streams;
  ow_init_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream>>>(plane, n_streams);
  return hipGetLastError();
}
hipError_t launch_output_writer_plan(const OwPush &p, hipStream_t stream) {
  ow_plan_kernel<<<dim3((unsigned)((p.n_streams + 63) / 64)), dim3(64), 0, stream>>>(p);
  return hipGetLastError();
}
hipError_t launch_output_writer_shape(const OwPush &p, hipStream_t stream) {
  ow_shape_kernel<<<dim3((unsigned)((p.max_out + kThreads - 1) / kThreads), (unsigned)p.n_streams), dim3(kThreads), 0, stream>>>(p);
  return hipGetLastError();
}
hipError_t launch_output_writer_gain(const OwPush &p, hipStream_t stream) {
  ow_gain_kernel<<<dim3((unsigned)((p.n_streams + 63) / 64)), dim3(64), 0, stream>>>(p);
  return hipGetLastError();
}
hipError_t launch_output_writer_out(const OwPush &p, hipStream_t stream) {
  ow_out_kernel<<<dim3((unsigned)((p.max_out + kThreads - 1) / kThreads), (unsigned)p.n_streams), dim3(kThreads), 0, stream>>>(p);
  return hipGetLastError();
}
hipError_t launch_output_writer_finish(const OwPush &p, hipStream_t stream) {
  ow_finish_kernel<<<dim3((unsigned)((p.n_streams + 63) / 64)), dim3(64), 0, stream>>>(p);
  return hipGetLastError();
}

}  // namespace af
