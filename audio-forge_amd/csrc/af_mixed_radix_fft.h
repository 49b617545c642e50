// af_mixed_radix_fft.h -- the in-LDS mixed-radix transform that the framed analyses share (af_noise_reference.hip,
// af_speech_features.hip): M complex f64 points whose length has no prime factor above 7, decimation in frequency with the
// outputs left in digit-reversed places, and the real transform of 2 M samples read off it.  Unfused f64; tables come from the
// host (nr_make_twiddles, nr_make_plan).  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "af_noise_reference_host.hpp"

namespace af {

__device__ inline double2 nr_cmul(double2 a, double2 t) { return make_double2(a.x * t.x - a.y * t.y, a.x * t.y + a.y * t.x); }

// One decimation-in-frequency stage of radix P over sub-transforms of length L = P * Ls: the butterfly at offset j of a block
// takes a[q] = buf[base + j + q Ls] and leaves (sum over q, in index order, of a[q] W_P^(q r)) W_L^(j r) at buf[base + j + r Ls].
// Output 0 needs no product; the others start from a[0] and multiply from q = 1 on.  tw[2 e] = exp(-2 pi i e / M).
template <int P>
__device__ void nr_stage(double2 *buf, int M, int L, const double2 *__restrict__ tw) {
  const int Ls = L / P, root = M / P, scale = M / L;
  for (int b = threadIdx.x; b < M / P; b += blockDim.x) {
    const int j = b % Ls, base = (b / Ls) * L + j;
    double2 a[P], y[P];
#pragma unroll
    for (int q = 0; q < P; ++q) a[q] = buf[base + q * Ls];
#pragma unroll
    for (int r = 0; r < P; ++r) {
      double2 acc = a[0];
#pragma unroll
      for (int q = 1; q < P; ++q) {
        const double2 t = r == 0 ? a[q] : nr_cmul(a[q], tw[2 * (((q * r) % P) * root)]);
        acc = make_double2(acc.x + t.x, acc.y + t.y);
      }
      y[r] = r == 0 ? acc : nr_cmul(acc, tw[2 * (j * r * scale)]);
    }
#pragma unroll
    for (int r = 0; r < P; ++r) buf[base + r * Ls] = y[r];
  }
  __syncthreads();
}

// every stage of the plan over buf[M], in the plan's order; the workgroup leaves it synchronised
__device__ inline void nr_transform(double2 *buf, int M, const NrPlan &plan, const double2 *__restrict__ tw) {
  for (int i = 0, L = M; i < plan.n_factors; ++i) {
    const int p = plan.factor[i];
    if (p == 2) nr_stage<2>(buf, M, L, tw);
    else if (p == 3) nr_stage<3>(buf, M, L, tw);
    else if (p == 5) nr_stage<5>(buf, M, L, tw);
    else nr_stage<7>(buf, M, L, tw);
    L /= p;
  }
}

// where Z[k] of the M-point transform ends: k = r1 + p1 (r2 + p2 (...)) sits at r1 M / p1 + r2 M / (p1 p2) + ...
__device__ inline int nr_digit_reverse(int k, int M, const NrPlan &plan) {
  int pos = 0, stride = M;
  for (int i = 0; i < plan.n_factors; ++i) {
    const int p = plan.factor[i];
    stride /= p;
    pos += (k % p) * stride;
    k /= p;
  }
  return pos;
}

// |X[k]|^2 of the real transform of the 2 M samples packed as (even, odd) pairs, from the half-length transform in buf, as
// vs_bin_power: tw[k] = exp(-2 pi i k / (2 M)), k = 0 .. M
__device__ inline double nr_real_bin_power(const double2 *buf, int k, int M, const NrPlan &plan, const double2 *__restrict__ tw) {
  const double2 a = buf[nr_digit_reverse(k % M, M, plan)], b = buf[nr_digit_reverse((M - k) % M, M, plan)], t = tw[k];
  const double er = 0.5 * (a.x + b.x), ei = 0.5 * (a.y - b.y);
  const double orr = 0.5 * (a.y + b.y), oi = -0.5 * (a.x - b.x);
  const double xr = er + (orr * t.x - oi * t.y), xi = ei + (orr * t.y + oi * t.x);
  return xr * xr + xi * xi;
}

}  // namespace af
