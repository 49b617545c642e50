// af_spectrum_stats.hip -- kernels of the reliability statistics behind the voice spectrum measurement, the second half of
// analyze_voice_spectrum (python/mic_eq/analysis/spectrum.py:250-290 _robust_median_spectrum, :381-495 _coarse_phonetic_coverage,
// _effective_block_count, _measurement_reliability).  Input is the smoothed dB rows vs_smooth_kernel leaves in the tile's scratch;
// what is O(windows) per stream (which windows are independent, blocks, inliers, percentiles, the scalars) is the host's, between
// two groups of launches (af_api_spectrum.cpp).  f64, unfused; medians select, sums run lane-strided and then down an xor tree,
// so two runs give the same bits.  tests/ref/voice_reliability_ref.c restates every operation in the same order.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "af_spectrum_host.hpp"

namespace af {
namespace {

constexpr int kVsStatThreads = 256;

__device__ double vs_wave_sum(double a) {
  for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off, 64);
  return a;
}

__device__ unsigned vs_pivot_hash(unsigned i, unsigned pass) {
  unsigned h = (i + 1u) * 2654435761u ^ pass * 0x9e3779b9u;
  h ^= h >> 15;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  return h;
}

// One wave, v[0 .. n) finite values in LDS: the k-th smallest (0-based) in every lane, and in *next the (k + 1)-th.  As
// vs_select: an open interval around the value narrows by one pivot per pass; every lane counts its stride of the values and
// the counts and the next pivots (the in-range value with the smallest hash) are reduced across the wave.
__device__ double vs_wave_select(const double *v, int n, int k, double *next) {
  const int lane = threadIdx.x & 63;
  double lo = -INFINITY, hi = INFINITY, pivot = v[n / 2];
  for (unsigned pass = 1; pass <= (unsigned)n + 1u; ++pass) {  // every pass removes its pivot from the interval
    int cl = 0, ce = 0;
    unsigned long long key_l = ~0ull, key_h = ~0ull;  // hash << 1: below every "no candidate"
    double cand_l = pivot, cand_h = pivot, above = INFINITY;
    for (int i = lane; i < n; i += 64) {
      const double x = v[i];
      cl += x < pivot;
      ce += x == pivot;
      const unsigned long long key = (unsigned long long)vs_pivot_hash((unsigned)i, pass) << 1;
      if (x > lo && x < pivot && key <= key_l) { key_l = key; cand_l = x; }
      if (x > pivot && x < hi && key <= key_h) { key_h = key; cand_h = x; }
      if (x > pivot && x < above) above = x;
    }
    for (int off = 32; off >= 1; off >>= 1) {
      cl += __shfl_xor(cl, off, 64);
      ce += __shfl_xor(ce, off, 64);
      const unsigned long long ol = __shfl_xor(key_l, off, 64), oh = __shfl_xor(key_h, off, 64);
      const double vl = __shfl_xor(cand_l, off, 64), vh = __shfl_xor(cand_h, off, 64), oa = __shfl_xor(above, off, 64);
      if (ol < key_l || (ol == key_l && vl < cand_l)) { key_l = ol; cand_l = vl; }
      if (oh < key_h || (oh == key_h && vh < cand_h)) { key_h = oh; cand_h = vh; }
      above = oa < above ? oa : above;
    }
    if (k >= cl && k < cl + ce) {  // wave-uniform: every lane holds the same counts
      *next = k + 1 < cl + ce ? pivot : above;
      return pivot;
    }
    if (k < cl) { hi = pivot; pivot = cand_l; } else { lo = pivot; pivot = cand_h; }
  }
  *next = pivot;  // not reached with finite values
  return pivot;
}

// np.median of v[0 .. n) by one wave
__device__ double vs_wave_median(const double *v, int n, double minus) {
  double b;
  const double a = vs_wave_select(v, n, (n - 1) / 2, &b);
  return (n & 1) ? a - minus : ((a - minus) + (b - minus)) / 2.0;
}

// One wave per smoothed row, the voice band staged in LDS: its mean (:440), its median (:268) and the coverage bands' medians
// of S - mean (:403).  Subtracting a row constant is monotone, so a band median is selected on S and the mean taken off the
// one or two selected values.
__global__ void __launch_bounds__(kVsStatThreads) vs_row_levels_kernel(const double *__restrict__ smooth, int32_t n_rows, int32_t bins,
                                                                        VsBandTable t, double *__restrict__ levels) {
  extern __shared__ double vs_band[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nb = t.v1 - t.v0 + 1;
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  const bool active = row < n_rows;
  double *v = vs_band + (size_t)wave * nb;
  if (active)
    for (int i = lane; i < nb; i += 64) v[i] = smooth[row * bins + t.v0 + i];
  __syncthreads();
  if (!active) return;  // whole waves leave together
  double a = 0.0;
  for (int i = lane; i < nb; i += 64) a += v[i];
  const double mean = vs_wave_sum(a) / (double)nb;
  const double median = vs_wave_median(v, nb, 0.0);
  double band[kVsCoverageBands];
  for (int b = 0; b < kVsCoverageBands; ++b) {
    const int n = t.last[b] - t.first[b] + 1;
    band[b] = n > 0 ? vs_wave_median(v + (t.first[b] - t.v0), n, mean) : NAN;
  }
  if (lane == 0) {
    double *out = levels + row * kVsLevelFields;
    out[0] = mean;
    out[1] = median;
    for (int b = 0; b < kVsCoverageBands; ++b) out[2 + b] = band[b];
  }
}

// vs_select over get(0 .. n): the k-th smallest by one thread, with its counts
template <class Get>
__device__ double vs_select_by(Get get, int n, int k, int *below, int *equal) {
  double lo = -INFINITY, hi = INFINITY, pivot = get(n / 2);
  for (unsigned pass = 1; pass <= (unsigned)n + 1u; ++pass) {
    int cl = 0, ce = 0;
    unsigned best_l = 0xffffffffu, best_h = 0xffffffffu;
    double cand_l = pivot, cand_h = pivot;
    for (int i = 0; i < n; ++i) {
      const double v = get(i);
      cl += v < pivot;
      ce += v == pivot;
      const unsigned h = vs_pivot_hash((unsigned)i, pass);
      if (v > lo && v < pivot && h <= best_l) { best_l = h; cand_l = v; }
      if (v > pivot && v < hi && h <= best_h) { best_h = h; cand_h = v; }
    }
    if (k >= cl && k < cl + ce) {
      *below = cl;
      *equal = ce;
      return pivot;
    }
    if (k < cl) { hi = pivot; pivot = cand_l; } else { lo = pivot; pivot = cand_h; }
  }
  *below = 0;  // not reached with finite values
  *equal = n;
  return pivot;
}

// np.median over get(0 .. n) by one thread
template <class Get>
__device__ double vs_median_by(Get get, int n) {
  int below, equal;
  const double a = vs_select_by(get, n, (n - 1) / 2, &below, &equal);
  if (n & 1) return a;
  double b = a;
  if (n / 2 >= below + equal) {  // the upper middle is the smallest value above a
    b = INFINITY;
    for (int i = 0; i < n; ++i) {
      const double v = get(i);
      if (v > a && v < b) b = v;
    }
  }
  return (a + b) / 2.0;
}

// vs_median_kernel over a row list with a value taken off every row: the offsets differ between rows, so the selection runs
// on the differences.  One thread per (job, bin); a workgroup's threads share the job, so jobs of different length do not
// wait for each other inside a workgroup.
__global__ void __launch_bounds__(kVsStatThreads) vs_offset_median_kernel(const double *__restrict__ smooth, const int32_t *__restrict__ list,
                                                                           const double *__restrict__ levels,
                                                                           const VsOffsetJob *__restrict__ jobs, int32_t bins,
                                                                           double *__restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= bins) return;
  const VsOffsetJob job = jobs[blockIdx.y];
  const int32_t *rows = list + job.first;
  double v = vs_median_by([&](int i) { return smooth[(int64_t)rows[i] * bins + k] - levels[(int64_t)rows[i] * kVsLevelFields + job.which]; },
                          job.count);
  if (job.with_add) v = v + job.add;
  out[(int64_t)job.out * bins + k] = v;
}

// One wave per smoothed row: the RMS over the voice band of the row's shape error against its stream's centre, :271-275
__global__ void __launch_bounds__(kVsStatThreads) vs_shape_distance_kernel(const double *__restrict__ smooth, int32_t n_rows, int32_t bins,
                                                                            int32_t v0, int32_t v1, const double *__restrict__ levels,
                                                                            const int32_t *__restrict__ row_centre,
                                                                            const double *__restrict__ centres, double *__restrict__ distance) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= n_rows) return;  // whole waves leave together
  const int32_t c = row_centre[row];
  if (c < 0) {
    if (lane == 0) distance[row] = NAN;
    return;
  }
  const double *s = smooth + row * bins, *centre = centres + (int64_t)c * bins;
  const double level = levels[row * kVsLevelFields + 1];
  double a = 0.0;
  for (int i = v0 + lane; i <= v1; i += 64) {
    const double d = (s[i] - level) - centre[i];
    a += d * d;
  }
  a = vs_wave_sum(a);
  if (lane == 0) distance[row] = sqrt(a / (double)(v1 - v0 + 1));
}

// One workgroup per stream over its block rows B[j][k].  Per bin the column median c, then with d_j = B[j][k] - c the lag-one
// sums of _effective_block_count (thread t takes bins t, t + 256, ..., pairs j in order; an xor tree per wave, the four waves
// in order) and 1.4826 median|d_j|; behind a barrier every thread derives the effective block count and finishes its bins.
__global__ void __launch_bounds__(kVsStatThreads) vs_block_stats_kernel(const double *__restrict__ block_rows, const VsBlockJob *__restrict__ jobs,
                                                                         int32_t bins, double *__restrict__ uncertainty,
                                                                         double *__restrict__ reliability, double *__restrict__ stats) {
  __shared__ double part[3 * (kVsStatThreads / 64)];
  const VsBlockJob job = jobs[blockIdx.x];
  const int nb = job.count, tid = threadIdx.x;
  const double *B = block_rows + (int64_t)job.row0 * bins;
  double *unc = uncertainty + (int64_t)job.out * bins, *rel = reliability + (int64_t)job.out * bins;
  if (nb < 2) {  // :466-468
    for (int k = tid; k < bins; k += kVsStatThreads) { unc[k] = INFINITY; rel[k] = 0.0; }
    if (tid == 0) {
      double *st = stats + (int64_t)job.out * 4;
      st[0] = st[1] = st[2] = 0.0;
      st[3] = (double)nb;  // :413-414
    }
    return;
  }
  double dot = 0.0, nl = 0.0, nr = 0.0;
  for (int k = tid; k < bins; k += kVsStatThreads) {
    const double c = vs_median_by([&](int j) { return B[(int64_t)j * bins + k]; }, nb);
    for (int j = 0; j + 1 < nb; ++j) {
      const double l = B[(int64_t)j * bins + k] - c, r = B[(int64_t)(j + 1) * bins + k] - c;
      dot += l * r;
      nl += l * l;
      nr += r * r;
    }
    unc[k] = 1.4826 * vs_median_by([&](int j) { return fabs(B[(int64_t)j * bins + k] - c); }, nb);  // robust sigma, finished below
  }
  dot = vs_wave_sum(dot);
  nl = vs_wave_sum(nl);
  nr = vs_wave_sum(nr);
  if ((tid & 63) == 0) {
    part[3 * (tid >> 6)] = dot;
    part[3 * (tid >> 6) + 1] = nl;
    part[3 * (tid >> 6) + 2] = nr;
  }
  __syncthreads();
  dot = part[0]; nl = part[1]; nr = part[2];
  for (int w = 1; w < kVsStatThreads / 64; ++w) { dot += part[3 * w]; nl += part[3 * w + 1]; nr += part[3 * w + 2]; }
  const double denominator = sqrt(nl) * sqrt(nr);
  double lag = 0.95;
  if (!(denominator <= 1e-12)) lag = fmin(fmax(dot / denominator, 0.0), 0.95);
  const double effective = fmin(fmax((double)nb * (1.0 - lag) / (1.0 + lag), 1.0), (double)nb);
  const double root = sqrt(fmax(effective, 1.0));
  for (int k = tid; k < bins; k += kVsStatThreads) {  // the bins this thread wrote above
    const double u = (1.253 * unc[k] + 0.35) / root, q = u / kVsUncertaintyScaleDb;
    unc[k] = u;
    rel[k] = fmin(fmax(exp(-(q * q)), 0.0), 1.0);
  }
  if (tid == 0) {
    double *st = stats + (int64_t)job.out * 4;
    st[0] = dot; st[1] = nl; st[2] = nr; st[3] = effective;
  }
}

}  // namespace

hipError_t launch_vs_row_levels(const double *smooth, int32_t n_rows, int32_t bins, const VsBandTable &bands, double *levels,
                                hipStream_t stream) {
  if (n_rows <= 0) return hipSuccess;
  const size_t band_bytes = sizeof(double) * (size_t)(bands.v1 - bands.v0 + 1);
  const int waves = (int)std::min<size_t>(kVsStatThreads / 64, std::max<size_t>(1, (size_t)65536 / band_bytes));  // 64 KB of LDS per workgroup
  hipLaunchKernelGGL(vs_row_levels_kernel, dim3((unsigned)((n_rows + waves - 1) / waves)), dim3(64 * waves), band_bytes * waves, stream,
                     smooth, n_rows, bins, bands, levels);
  return hipGetLastError();
}

hipError_t launch_vs_offset_median(const double *smooth, const int32_t *list, const double *levels, const VsOffsetJob *jobs,
                                   int32_t n_jobs, int32_t bins, double *out, hipStream_t stream) {
  if (n_jobs <= 0) return hipSuccess;
  for (int32_t j0 = 0; j0 < n_jobs; j0 += 65535) {  // gridDim.y
    const int32_t nj = std::min(n_jobs - j0, 65535);
    hipLaunchKernelGGL(vs_offset_median_kernel, dim3((unsigned)((bins + kVsStatThreads - 1) / kVsStatThreads), (unsigned)nj),
                       dim3(kVsStatThreads), 0, stream, smooth, list, levels, jobs + j0, bins, out);
  }
  return hipGetLastError();
}

hipError_t launch_vs_shape_distance(const double *smooth, int32_t n_rows, int32_t bins, const VsBandTable &bands, const double *levels,
                                    const int32_t *row_centre, const double *centres, double *distance, hipStream_t stream) {
  if (n_rows <= 0) return hipSuccess;
  const int waves = kVsStatThreads / 64;
  hipLaunchKernelGGL(vs_shape_distance_kernel, dim3((unsigned)((n_rows + waves - 1) / waves)), dim3(kVsStatThreads), 0, stream, smooth,
                     n_rows, bins, bands.v0, bands.v1, levels, row_centre, centres, distance);
  return hipGetLastError();
}

hipError_t launch_vs_block_stats(const double *block_rows, const VsBlockJob *jobs, int32_t n_jobs, int32_t bins, double *uncertainty,
                                 double *reliability, double *stats, hipStream_t stream) {
  if (n_jobs <= 0) return hipSuccess;
  hipLaunchKernelGGL(vs_block_stats_kernel, dim3((unsigned)n_jobs), dim3(kVsStatThreads), 0, stream, block_rows, jobs, bins, uncertainty,
                     reliability, stats);
  return hipGetLastError();
}

}  // namespace af
