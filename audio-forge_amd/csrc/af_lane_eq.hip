// af_lane_eq.hip -- the 10-band EQ with PER-LANE section coefficients over shared captures.
//
// lane_eq_kernel: a lane is one (capture, band set) pair, a wave is 64 lanes, a workgroup is one wave.  Every lane runs what
//   chain_lane_kernel (af_kernels.hip) runs for an EQ-only chain -- the input scrub, then biquad_tile's operations per section:
//   f64 DF2T, the result rounded to f32 after every section, the parallel-state coefficient crossfade and its promotion
//   (dsp/biquad.rs:263-327) -- from zero state, strictly sample-sequential: its output equals the engine's bit for bit.
//   What the engine reads from its uniform parameter block through scalar loads is per lane here: the active coefficients
//   (50 doubles) and the filter memories (20 doubles, 20 more for the pending filters) live in VGPRs for the whole launch;
//   the pending coefficients are fetched from the planes only in tiles where some lane still crossfades.  The crossfade
//   position is per lane and per section (a setter may have scheduled nothing), so no `rem` is assumed wave-uniform.
//   Audio moves through a 64 x 65 f32 LDS tile in both directions: row r of the tile is one coalesced 256 B read of lane r's
//   capture (consecutive lanes that share a capture share the read) and one coalesced 256 B write of lane r's output row;
//   in between lane i walks column i, conflict free.
//   The tiles up to the last one in which a lane of the wave crossfades (two at 48 kHz: 72 samples) run band-major like the
//   engine (one section over the tile, then the next); all later tiles run sample-major with the ten sections unrolled, which leaves the compiler section k's memory updates to fill the
//   latency of section k+1's dependent chain.  A section's output depends only on its own input sequence, so both orders
//   give the same bits.
#include <hip/hip_runtime.h>

#include "af_dsp.h"
#include "af_lane_eq_host.hpp"

namespace af {

// capture rows -> tile, transposed; non-finite input is zeroed as the engine does (python_api.rs:517-520)
__device__ __forceinline__ void le_load_tile(const LaneEqArgs &a, float (*x)[kLanes + 1], int64_t t0, int len, int g0, int lane) {
  int loaded = -1;
  float v = 0.0f;
#pragma unroll 4
  for (int r = 0; r < kLanes; ++r) {
    const int cap = a.lane_capture[g0 + r];  // wave-uniform
    if (cap != loaded) {
      v = lane < len ? a.in[(int64_t)cap * a.in_stride + t0 + lane] : 0.0f;
      if (!finite_f32(v)) v = 0.0f;
      loaded = cap;
    }
    x[lane][r] = v;
  }
  __syncthreads();
}

// tile -> output rows: 256 B of one lane's row per instruction
__device__ __forceinline__ void le_store_tile(const LaneEqArgs &a, float (*x)[kLanes + 1], int64_t t0, int len, int g0, int lane) {
  __syncthreads();
  if (lane < len) {
#pragma unroll 8
    for (int r = 0; r < kLanes; ++r)
      if (g0 + r < a.n_lanes) a.out[(int64_t)(g0 + r) * a.out_stride + t0 + lane] = x[lane][r];
  }
  __syncthreads();
}

extern "C" __global__ __launch_bounds__(kLanes) void lane_eq_kernel(LaneEqArgs a) {
  __shared__ float x[kTile][kLanes + 1];

  const int lane = threadIdx.x;
  const int g0 = blockIdx.x * kLanes;
  const int g = g0 + lane;  // < lanes_padded: every per-lane plane and the output rows are padded to whole waves
  const int64_t LP = a.lanes_padded;
  const int64_t n = a.n_samples;

  BiquadCoef c[kLeSections];
  double z1[kLeSections], z2[kLeSections];
  int64_t t0 = 0;
  {
    // ---- the crossfade phase: while some lane of the wave crossfades, band-major like the engine -- biquad_tile with a
    //      per-lane `rem`.  The pending coefficients and memories live only here.
    double pz1[kLeSections], pz2[kLeSections];
    int rem[kLeSections];
    bool fading = false;
#pragma unroll
    for (int k = 0; k < kLeSections; ++k) {
      const double *f = a.coef + (int64_t)(10 * k) * LP + g;
      c[k] = BiquadCoef{f[0], f[LP], f[2 * LP], f[3 * LP], f[4 * LP]};
      z1[k] = z2[k] = pz1[k] = pz2[k] = 0.0;
      rem[k] = a.fade[(int64_t)(2 * k + 1) * LP + g];
      fading |= rem[k] > 0;
    }
    for (; t0 < n && __ballot(fading) != 0; t0 += kTile) {
      const int len = (int)((n - t0) < kTile ? (n - t0) : kTile);
      le_load_tile(a, x, t0, len, g0, lane);
      fading = false;
#pragma unroll
      for (int k = 0; k < kLeSections; ++k) {
        const double *f = a.coef + (int64_t)(10 * k + 5) * LP + g;
        const BiquadCoef p{f[0], f[LP], f[2 * LP], f[3 * LP], f[4 * LP]};
        const int xf_total = a.fade[(int64_t)(2 * k) * LP + g];
        const double total = (double)xf_total;
#pragma nounroll
        for (int t = 0; t < len; ++t) {
          const double in = (double)x[t][lane];
          double y;
          if (rem[k] > 0) {
            const double ya = c[k].b0 * in + z1[k];
            z1[k] = c[k].b1 * in - c[k].a1 * ya + z2[k];
            z2[k] = c[k].b2 * in - c[k].a2 * ya;
            const double yp = p.b0 * in + pz1[k];
            pz1[k] = p.b1 * in - p.a1 * yp + pz2[k];
            pz2[k] = p.b2 * in - p.a2 * yp;
            const int fade_pos = xf_total - rem[k] + 1;
            const double fade = (double)fade_pos / total;
            y = ya * (1.0 - fade) + yp * fade;
            rem[k] -= 1;
            if (rem[k] == 0) {  // promote_pending_coefficients, biquad.rs:276-286
              c[k] = p;
              z1[k] = pz1[k];
              z2[k] = pz2[k];
            }
          } else {
            y = c[k].b0 * in + z1[k];
            z1[k] = c[k].b1 * in - c[k].a1 * y + z2[k];
            z2[k] = c[k].b2 * in - c[k].a2 * y;
          }
          x[t][lane] = (float)y;
        }
        fading |= rem[k] > 0;
      }
      le_store_tile(a, x, t0, len, g0, lane);
    }
  }

  // ---- the steady loop: sample-major, 50 coefficients and 20 memories in registers
  for (; t0 < n; t0 += kTile) {
    const int len = (int)((n - t0) < kTile ? (n - t0) : kTile);
    le_load_tile(a, x, t0, len, g0, lane);
#pragma nounroll
    for (int t = 0; t < len; ++t) {
      float v = x[t][lane];
#pragma unroll
      for (int k = 0; k < kLeSections; ++k) {
        const double in = (double)v;
        const double y = c[k].b0 * in + z1[k];
        z1[k] = c[k].b1 * in - c[k].a1 * y + z2[k];
        z2[k] = c[k].b2 * in - c[k].a2 * y;
        v = (float)y;
      }
      x[t][lane] = v;
    }
    le_store_tile(a, x, t0, len, g0, lane);
  }
}

hipError_t launch_lane_eq(const LaneEqArgs &args, hipStream_t stream) {
  hipLaunchKernelGGL(lane_eq_kernel, dim3(args.lanes_padded / kLanes), dim3(kLanes), 0, stream, args);
  return hipGetLastError();
}

}  // namespace af
