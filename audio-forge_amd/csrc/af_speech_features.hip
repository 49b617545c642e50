// af_speech_features.hip -- kernels of the speech-feature measurement (python/mic_eq/analysis/voice_setup.py:161-458) at 48 kHz:
// frame powers, K-weighted energies on the hop grid, one Hann-windowed real FFT of 1920 samples per listed frame with its band
// sums and the sibilance band's maximum, arg-max and median, and the probability-weighted candidate spectrum with its peak.
// All arithmetic is f64 and unfused (-ffp-contract=off) and everything left is linear: the host takes the decibels.
// tests/ref/speech_features_ref.c restates every operation in the same order.  The transform is af_mixed_radix_fft.h's; the
// medians over frames are af_spectrum.hip's launch_vs_median.
#include <hip/hip_runtime.h>

#include "af_mixed_radix_fft.h"
#include "af_speech_features_host.hpp"

namespace af {
namespace {

constexpr int kSfLanes = 64, kSfTile = 64;
constexpr int kSfMinStreamsPerGroup = 16, kSfComputeUnits = 256;  // sf_kweight_kernel's streams per workgroup: 64, or down to 16
constexpr int kSfMaxSibBins = 512;

__device__ inline double sf_wave_sum(double v) {  // every lane ends with the same total
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ void __launch_bounds__(kSfThreads) sf_frame_power_kernel(const float *__restrict__ audio, int64_t stride, int64_t total,
                                                                     int32_t n_frames, double *__restrict__ power) {
  const int lane = threadIdx.x & 63;
  const int64_t id = (int64_t)blockIdx.x * (kSfThreads / 64) + (threadIdx.x >> 6);
  if (id >= total) return;  // whole waves leave together
  const int64_t s = id / n_frames, f = id % n_frames;
  const float *x = audio + s * stride + f * kSfHop;
  double q = 0.0;
  for (int i = lane; i < kSfFrame; i += 64) {
    const double v = (double)x[i];
    q += v * v;
  }
  q = sf_wave_sum(q);
  if (lane == 0) power[id] = q / (double)kSfFrame;
}

// lfilter's step for one second-order section (a0 = 1): y = z0 + b0 x; z0 = (z1 + b1 x) - a1 y; z1 = b2 x - a2 y
__device__ inline double sf_section(double b0, double b1, double b2, double a1, double a2, double x, double &z0, double &z1) {
  const double y = z0 + b0 * x;
  z0 = (z1 + b1 * x) - a1 * y;
  z1 = b2 * x - a2 * y;
  return y;
}

// `per` streams a workgroup (at most 64, one lane each): the launcher takes fewer than 64 when whole workgroups of 64 would leave
// compute units idle.  A stream's arithmetic does not depend on it.
__global__ void __launch_bounds__(kSfLanes) sf_kweight_kernel(const float *__restrict__ audio, int64_t stride, int64_t n, int32_t n_streams,
                                                               int32_t n_chunks, int32_t per, double *__restrict__ energy) {
  __shared__ float x[kSfTile][kSfLanes + 1];
  const int lane = threadIdx.x, s0 = blockIdx.x * per, s = s0 + lane, column = lane < per ? lane : 0;
  const bool valid = lane < per && s < n_streams;
  double a0 = 0.0, a1 = 0.0, h0 = 0.0, h1 = 0.0, acc = 0.0;
  int in_chunk = 0, chunk = 0;
  for (int64_t t0 = 0; t0 < n; t0 += kSfTile) {
    const int len = (int)((n - t0) < kSfTile ? (n - t0) : kSfTile);
    for (int r = 0; r < per; ++r) {
      const int sr = s0 + r;
      float v = 0.0f;
      if (sr < n_streams && lane < len) v = audio[(int64_t)sr * stride + t0 + lane];
      x[lane][r] = v;
    }
    __syncthreads();
    for (int t = 0; t < len; ++t) {
      const double shelved = sf_section(kSfShelf[0], kSfShelf[1], kSfShelf[2], kSfShelf[3], kSfShelf[4], (double)x[t][column], a0, a1);
      const double y = sf_section(kSfHighpass[0], kSfHighpass[1], kSfHighpass[2], kSfHighpass[3], kSfHighpass[4], shelved, h0, h1);
      acc += y * y;
      if (++in_chunk == kSfHop) {
        if (valid && chunk < n_chunks) energy[(int64_t)s * n_chunks + chunk] = acc;
        acc = 0.0;
        in_chunk = 0;
        ++chunk;
      }
    }
    __syncthreads();
  }
  if (in_chunk > 0 && valid && chunk < n_chunks) energy[(int64_t)s * n_chunks + chunk] = acc;  // the partial tail
}

__global__ void __launch_bounds__(kSfThreads) sf_frame_kernel(const float *__restrict__ speech, int64_t speech_stride,
                                                               const float *__restrict__ noise, int64_t noise_stride,
                                                               const SfFrameItem *__restrict__ items, NrPlan plan, SfBandTable bands,
                                                               const double *__restrict__ window, const double2 *__restrict__ tw,
                                                               double *__restrict__ band, double *__restrict__ sib_mid,
                                                               int32_t *__restrict__ sib_arg, double *__restrict__ sib_rows,
                                                               double *__restrict__ noise_band) {
  __shared__ double2 buf[kSfHop];  // the half-length transform; the power row as doubles once it has been read
  __shared__ double wave_total[kSfThreads / 64];
  const SfFrameItem it = items[blockIdx.x];
  constexpr int M = kSfHop, T = kSfThreads;
  const int tid = threadIdx.x;
  const float *x = (it.source ? speech + (int64_t)it.stream * speech_stride : noise + (int64_t)it.stream * noise_stride) + (int64_t)it.chunk * kSfHop;
  double sum = 0.0;  // np.mean(frame), :280: strided partial sums, an xor tree per wave, the waves in order
  for (int i = tid; i < kSfFrame; i += T) sum += (double)x[i];
  sum = sf_wave_sum(sum);
  if ((tid & 63) == 0) wave_total[tid >> 6] = sum;
  __syncthreads();
  const double mean = (((wave_total[0] + wave_total[1]) + wave_total[2]) + wave_total[3]) / (double)kSfFrame;
  for (int m = tid; m < M; m += T)
    buf[m] = make_double2(((double)x[2 * m] - mean) * window[2 * m], ((double)x[2 * m + 1] - mean) * window[2 * m + 1]);
  __syncthreads();
  nr_transform(buf, M, plan, tw);
  double p[(M + T) / T];  // bins tid, tid + T, ...: M + 1 of them in all
#pragma unroll
  for (int j = 0; j < (M + T) / T; ++j) {
    const int k = tid + j * T;
    p[j] = k <= M ? nr_real_bin_power(buf, k, M, plan, tw) + 1e-18 : 0.0;
  }
  __syncthreads();  // every read of the transform is done: the buffer now takes the row
  double *pw = reinterpret_cast<double *>(buf);
#pragma unroll
  for (int j = 0; j < (M + T) / T; ++j) {
    const int k = tid + j * T;
    if (k <= M) pw[k] = p[j];
  }
  __syncthreads();
  const int s0 = bands.first[kSfSibBand], ns = bands.last[kSfSibBand] - s0 + 1;
  if (!it.source) {  // a noise frame: the 5000-9500 Hz sum only, :337
    if (tid == 0) {
      double s = 0.0;
      for (int k = 0; k < ns; ++k) s += pw[s0 + k];
      noise_band[it.row] = s;
    }
    return;
  }
  if (tid < kSfBands) {  // one thread a band, in bin order
    double s = 0.0;
    for (int k = bands.first[tid]; k <= bands.last[tid]; ++k) s += pw[k];
    band[(int64_t)it.row * kSfBandFields + tid] = s;
  } else if (tid == kSfBands) {  // np.max and np.argmax (the first) over the sibilance bins, :352-354
    double top = pw[s0];
    int arg = 0;
    for (int k = 1; k < ns; ++k)
      if (pw[s0 + k] > top) { top = pw[s0 + k]; arg = k; }
    band[(int64_t)it.row * kSfBandFields + kSfBands] = top;
    band[(int64_t)it.row * kSfBandFields + kSfBands + 1] = 0.0;
    sib_arg[it.row] = arg;
  }
  for (int k = tid; k < ns; k += T) {  // the row for the candidate spectrum, and the median by rank: ties are ordered by index
    const double v = pw[s0 + k];
    int rank = 0;
    for (int j = 0; j < ns; ++j) {
      const double u = pw[s0 + j];
      rank += (u < v) || (u == v && j < k);
    }
    sib_rows[(int64_t)it.row * ns + k] = v;
    if (rank == (ns - 1) / 2) sib_mid[(int64_t)it.row * 2] = v;
    if (rank == ns / 2) sib_mid[(int64_t)it.row * 2 + 1] = v;
  }
}

__global__ void __launch_bounds__(kSfThreads) sf_weighted_peak_kernel(const double *__restrict__ sib_rows, const double *__restrict__ weights,
                                                                       const SfPeakJob *__restrict__ jobs, int32_t ns,
                                                                       double *__restrict__ sums, int32_t *__restrict__ arg) {
  __shared__ double row[kSfMaxSibBins];
  const SfPeakJob job = jobs[blockIdx.x];
  for (int k = threadIdx.x; k < ns; k += blockDim.x) {  // np.average(axis=0, weights=): one addition per frame, in frame order
    double acc = 0.0;
    for (int i = 0; i < job.count; ++i) acc += weights[job.row0 + i] * sib_rows[(int64_t)(job.row0 + i) * ns + k];
    row[k] = acc;
    sums[(int64_t)job.out * ns + k] = acc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int best = 0;
    for (int k = 1; k < ns; ++k)
      if (row[k] > row[best]) best = k;
    arg[job.out] = best;
  }
}

}  // namespace

hipError_t launch_sf_frame_power(const float *audio, int64_t stride, int32_t n_streams, int32_t n_frames, double *power, hipStream_t stream) {
  const int64_t total = (int64_t)n_streams * n_frames, per = kSfThreads / 64;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(sf_frame_power_kernel, dim3((unsigned)((total + per - 1) / per)), dim3(kSfThreads), 0, stream, audio, stride, total,
                     n_frames, power);
  return hipGetLastError();
}

hipError_t launch_sf_kweight(const float *audio, int64_t stride, int64_t n, int32_t n_streams, int32_t n_chunks, double *energy,
                             hipStream_t stream) {
  if (n_streams <= 0 || n <= 0) return hipSuccess;
  int per = kSfLanes;  // the recurrence is latency-bound: spread a small batch over the compute units before filling the lanes
  while (per > kSfMinStreamsPerGroup && (n_streams + per - 1) / per < kSfComputeUnits) per /= 2;
  hipLaunchKernelGGL(sf_kweight_kernel, dim3((unsigned)((n_streams + per - 1) / per)), dim3(kSfLanes), 0, stream, audio, stride, n,
                     n_streams, n_chunks, per, energy);
  return hipGetLastError();
}

hipError_t launch_sf_frames(const float *speech, int64_t speech_stride, const float *noise, int64_t noise_stride, const SfFrameItem *items,
                            int32_t n_items, const NrPlan &plan, const SfBandTable &bands, const double *window, const double *twiddles,
                            double *band, double *sib_mid, int32_t *sib_arg, double *sib_rows, double *noise_band, hipStream_t stream) {
  if (n_items <= 0) return hipSuccess;
  hipLaunchKernelGGL(sf_frame_kernel, dim3((unsigned)n_items), dim3(kSfThreads), 0, stream, speech, speech_stride, noise, noise_stride, items,
                     plan, bands, window, (const double2 *)twiddles, band, sib_mid, sib_arg, sib_rows, noise_band);
  return hipGetLastError();
}

hipError_t launch_sf_weighted_peak(const double *sib_rows, const double *weights, const SfPeakJob *jobs, int32_t n_jobs, int32_t sib_bins,
                                   double *sums, int32_t *arg, hipStream_t stream) {
  if (n_jobs <= 0) return hipSuccess;
  if (sib_bins <= 0 || sib_bins > kSfMaxSibBins) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sf_weighted_peak_kernel, dim3((unsigned)n_jobs), dim3(kSfThreads), 0, stream, sib_rows, weights, jobs, sib_bins, sums,
                     arg);
  return hipGetLastError();
}

}  // namespace af
