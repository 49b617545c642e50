// af_noise_reference.hip -- kernels of the room-noise reference analysis (python/mic_eq/analysis/noise_reference.py): sample
// statistics of the noise capture, chunk sums and centred frame powers of both captures, and a Hann-windowed real FFT of one
// frame per workgroup whose length need not be a power of two (the frame is 0.2 s: 9600 samples at 48 kHz), with the octave-band
// sums behind it.  All arithmetic is f64 and unfused (-ffp-contract=off); window, twiddles, factor list and band ranges come from
// the host.  A non-finite sample reads as 0 (:294-297, :416).  tests/ref/noise_reference_ref.c restates every operation in the
// same order.  The column medians over the PSD rows are af_spectrum.hip's launch_vs_median.
#include <hip/hip_runtime.h>

#include "af_mixed_radix_fft.h"
#include "af_noise_reference_host.hpp"

namespace af {
namespace {

__device__ inline double nr_sample(const float *x, int64_t i) {
  const float v = x[i];
  return isfinite(v) ? (double)v : 0.0;
}

__device__ inline double nr_wave_sum(double v) {  // every lane ends with the same total
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ void __launch_bounds__(kNrThreads) nr_sample_stats_kernel(const float *__restrict__ audio, int64_t stride, int64_t n,
                                                                      int32_t n_streams, NrSampleStats *__restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * (kNrThreads / 64) + (threadIdx.x >> 6);
  if (s >= n_streams) return;  // whole waves leave together
  const float *x = audio + s * stride;
  double q = 0.0, peak = 0.0;
  long long finite = 0, clipped = 0, zero = 0;
  for (int64_t i = lane; i < n; i += 64) {
    const float raw = x[i];
    const bool ok = isfinite(raw);
    const double v = ok ? (double)raw : 0.0, a = fabs(v);
    finite += ok;
    q += v * v;
    peak = a > peak ? a : peak;
    clipped += a >= 0.999;
    zero += a <= 1e-12;
  }
  q = nr_wave_sum(q);
  for (int off = 32; off >= 1; off >>= 1) {
    const double other = __shfl_xor(peak, off, 64);
    peak = other > peak ? other : peak;
    finite += __shfl_xor(finite, off, 64);
    clipped += __shfl_xor(clipped, off, 64);
    zero += __shfl_xor(zero, off, 64);
  }
  if (lane == 0) stats[s] = NrSampleStats{q, peak, (int64_t)finite, (int64_t)clipped, (int64_t)zero};
}

__global__ void __launch_bounds__(kNrThreads) nr_chunk_sums_kernel(const float *__restrict__ audio, int64_t stride, int64_t total,
                                                                    int32_t n_chunks, int32_t hop, double *__restrict__ sums) {
  const int lane = threadIdx.x & 63;
  const int64_t id = (int64_t)blockIdx.x * (kNrThreads / 64) + (threadIdx.x >> 6);
  if (id >= total) return;
  const int64_t s = id / n_chunks, c = id % n_chunks;
  const float *x = audio + s * stride + c * hop;
  double a = 0.0, q = 0.0;
  for (int i = lane; i < hop; i += 64) {
    const double v = nr_sample(x, i);
    a += v;
    q += v * v;
  }
  a = nr_wave_sum(a);
  q = nr_wave_sum(q);
  if (lane == 0) {
    sums[id * 2] = a;
    sums[id * 2 + 1] = q;
  }
}

__global__ void __launch_bounds__(kNrThreads) nr_frame_power_kernel(const float *__restrict__ audio, int64_t stride,
                                                                     const double *__restrict__ sums, int64_t total, int32_t n_frames,
                                                                     int32_t hop, double *__restrict__ power) {
  const int lane = threadIdx.x & 63;
  const int64_t id = (int64_t)blockIdx.x * (kNrThreads / 64) + (threadIdx.x >> 6);
  if (id >= total) return;
  const int64_t s = id / n_frames, f = id % n_frames;
  const int N = 2 * hop;
  const float *x = audio + s * stride + f * hop;
  const double *sm = sums + (s * (n_frames + 1) + f) * 2;
  const double mean = (sm[0] + sm[2]) / (double)N;
  double q = 0.0;
  for (int i = lane; i < N; i += 64) {
    const double d = nr_sample(x, i) - mean;
    q += d * d;
  }
  q = nr_wave_sum(q);
  if (lane == 0) power[id] = q / (double)N;
}

__global__ void __launch_bounds__(kNrThreads) nr_frame_kernel(const float *__restrict__ noise, int64_t noise_stride,
                                                               const double *__restrict__ noise_sums, int32_t noise_chunks,
                                                               const float *__restrict__ voice, int64_t voice_stride,
                                                               const double *__restrict__ voice_sums, int32_t voice_chunks,
                                                               const NrFrameItem *__restrict__ items, int32_t frame, NrPlan plan,
                                                               NrBandTable bands, const double *__restrict__ window,
                                                               const double2 *__restrict__ tw, double sumw2, double *__restrict__ psd,
                                                               double *__restrict__ band_power) {
  extern __shared__ double2 nr_buf[];  // [M]; the PSD as doubles once the transform has been read
  const NrFrameItem it = items[blockIdx.x];
  const int N = frame, M = N / 2, tid = threadIdx.x, T = blockDim.x;
  const float *x = (it.source ? voice + (int64_t)it.stream * voice_stride : noise + (int64_t)it.stream * noise_stride) + (int64_t)it.chunk * M;
  const double *sm = it.source ? voice_sums + ((int64_t)it.stream * voice_chunks + it.chunk) * 2
                               : noise_sums + ((int64_t)it.stream * noise_chunks + it.chunk) * 2;
  const double mean = (sm[0] + sm[2]) / (double)N;
  for (int m = tid; m < M; m += T)
    nr_buf[m] = make_double2((nr_sample(x, 2 * m) - mean) * window[2 * m], (nr_sample(x, 2 * m + 1) - mean) * window[2 * m + 1]);
  __syncthreads();
  nr_transform(nr_buf, M, plan, tw);
  // the real transform from the half-length one, as vs_bin_power: tw[k] = exp(-2 pi i k / N)
  double *row = psd + (int64_t)it.row * (M + 1);
  for (int k = tid; k <= M; k += T) row[k] = nr_real_bin_power(nr_buf, k, M, plan, tw) / sumw2;
  __syncthreads();  // every read of the transform is done: the buffer now takes the row, for the band sums
  double *pw = reinterpret_cast<double *>(nr_buf);
  for (int k = tid; k <= M; k += T) pw[k] = row[k];  // each thread reads back what it wrote
  __syncthreads();
  if (tid < kNrBands) {  // one thread a band, in bin order; 0 behind the bands that hold a bin
    double s = 0.0;
    if (tid < bands.n_bands)
      for (int k = bands.first[tid]; k <= bands.last[tid]; ++k) s += pw[k];
    band_power[(int64_t)it.row * kNrBands + tid] = s;
  }
}

}  // namespace

hipError_t launch_nr_sample_stats(const float *audio, int64_t stride, int64_t n, int32_t n_streams, NrSampleStats *stats,
                                  hipStream_t stream) {
  if (n_streams <= 0) return hipSuccess;
  const int per = kNrThreads / 64;
  hipLaunchKernelGGL(nr_sample_stats_kernel, dim3((unsigned)((n_streams + per - 1) / per)), dim3(kNrThreads), 0, stream, audio, stride, n,
                     n_streams, stats);
  return hipGetLastError();
}

hipError_t launch_nr_chunk_sums(const float *audio, int64_t stride, int32_t n_streams, int32_t n_chunks, int32_t hop, double *sums,
                                hipStream_t stream) {
  const int64_t total = (int64_t)n_streams * n_chunks, per = kNrThreads / 64;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(nr_chunk_sums_kernel, dim3((unsigned)((total + per - 1) / per)), dim3(kNrThreads), 0, stream, audio, stride, total,
                     n_chunks, hop, sums);
  return hipGetLastError();
}

hipError_t launch_nr_frame_power(const float *audio, int64_t stride, const double *sums, int32_t n_streams, int32_t n_frames,
                                 int32_t hop, double *power, hipStream_t stream) {
  const int64_t total = (int64_t)n_streams * n_frames, per = kNrThreads / 64;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(nr_frame_power_kernel, dim3((unsigned)((total + per - 1) / per)), dim3(kNrThreads), 0, stream, audio, stride, sums,
                     total, n_frames, hop, power);
  return hipGetLastError();
}

hipError_t launch_nr_frame_spectra(const float *noise, int64_t noise_stride, const double *noise_sums, int32_t noise_chunks,
                                   const float *voice, int64_t voice_stride, const double *voice_sums, int32_t voice_chunks,
                                   const NrFrameItem *items, int32_t n_items, int32_t frame, const NrPlan &plan, const NrBandTable &bands,
                                   const double *window, const double *twiddles, double sumw2, double *psd, double *band_power,
                                   hipStream_t stream) {
  if (n_items <= 0) return hipSuccess;
  const size_t lds = sizeof(double2) * (size_t)(frame / 2);  // M + 1 doubles fit in it from M = 1 on
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(nr_frame_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         160 * 1024);
    if (err != hipSuccess) return err;
    attr_set = true;
  }
  hipLaunchKernelGGL(nr_frame_kernel, dim3((unsigned)n_items), dim3(kNrThreads), lds, stream, noise, noise_stride, noise_sums,
                     noise_chunks, voice, voice_stride, voice_sums, voice_chunks, items, frame, plan, bands, window,
                     (const double2 *)twiddles, sumw2, psd, band_power);
  return hipGetLastError();
}

}  // namespace af
