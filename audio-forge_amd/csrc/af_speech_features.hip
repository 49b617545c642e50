// af_speech_features.hip -- kernels of the speech-feature measurement (python/mic_eq/analysis/voice_setup.py:161-458) at 48 kHz:
// frame powers, K-weighted energies on the hop grid, one Hann-windowed real FFT of 1920 samples per listed frame with its band
// sums and the sibilance band's maximum, arg-max and median, and the probability-weighted candidate spectrum with its peak.
// All arithmetic is f64 and unfused (-ffp-contract=off) and everything left is linear: the host takes the decibels.
// tests/ref/speech_features_ref.c restates every operation in the same order.  The transform is af_mixed_radix_fft.h's; the
// medians over frames are af_spectrum.hip's launch_vs_median.
// Frame, hop, plan, window, twiddles and band table are arguments: 1920 / 960 at 48 kHz, the geometry of the capture's rate behind
// af_device_rate_features_*, whose captures sf_resample_kernel takes to 48 kHz (scipy.signal.resample_poly's polyphase sum, the
// oldest input first) in front of the K-weighting.
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
                                                                     int32_t n_frames, int32_t frame, int32_t hop, double *__restrict__ power) {
  const int lane = threadIdx.x & 63;
  const int64_t id = (int64_t)blockIdx.x * (kSfThreads / 64) + (threadIdx.x >> 6);
  if (id >= total) return;  // whole waves leave together
  const int64_t s = id / n_frames, f = id % n_frames;
  const float *x = audio + s * stride + f * hop;
  double q = 0.0;
  for (int i = lane; i < frame; i += 64) {
    const double v = (double)x[i];
    q += v * v;
  }
  q = sf_wave_sum(q);
  if (lane == 0) power[id] = q / (double)frame;
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
// In: float for a 48 kHz capture, double for a resampled one.  Masked: the resampled form, which runs over one segment of whole
// chunks at a time (the scratch holds every stream's segment, so that all streams stay side by side: the recurrence is serial in
// time): it takes up the four filter states of state[s] and leaves them there, counts chunks from chunk0, and also sums the
// energy behind mask[s][t] (the resampled activity mask as bytes) per chunk, for the loudness fallback of :243-249.  The float
// form is what it was.
template <typename In, bool Masked>
__global__ void __launch_bounds__(kSfLanes) sf_kweight_kernel(const In *__restrict__ audio, int64_t stride, int64_t n, int32_t n_streams,
                                                               int32_t n_chunks, int32_t per, double *__restrict__ energy,
                                                               const uint8_t *__restrict__ mask, double *__restrict__ masked_energy,
                                                               double *__restrict__ state, int32_t chunk0) {
  __shared__ In x[kSfTile][kSfLanes + 1];
  __shared__ uint8_t on[Masked ? kSfTile : 1][kSfLanes + 1];
  double masked_acc = 0.0;
  const int lane = threadIdx.x, s0 = blockIdx.x * per, s = s0 + lane, column = lane < per ? lane : 0;
  const bool valid = lane < per && s < n_streams;
  double a0 = 0.0, a1 = 0.0, h0 = 0.0, h1 = 0.0, acc = 0.0;
  int in_chunk = 0, chunk = Masked ? chunk0 : 0;
  if (Masked && valid) { a0 = state[4 * s]; a1 = state[4 * s + 1]; h0 = state[4 * s + 2]; h1 = state[4 * s + 3]; }
  for (int64_t t0 = 0; t0 < n; t0 += kSfTile) {
    const int len = (int)((n - t0) < kSfTile ? (n - t0) : kSfTile);
    for (int r = 0; r < per; ++r) {
      const int sr = s0 + r;
      In v = (In)0;
      if (sr < n_streams && lane < len) v = audio[(int64_t)sr * stride + t0 + lane];
      x[lane][r] = v;
      if (Masked) on[lane][r] = sr < n_streams && lane < len ? mask[(int64_t)sr * stride + t0 + lane] : 0;
    }
    __syncthreads();
    for (int t = 0; t < len; ++t) {
      const double shelved = sf_section(kSfShelf[0], kSfShelf[1], kSfShelf[2], kSfShelf[3], kSfShelf[4], (double)x[t][column], a0, a1);
      const double y = sf_section(kSfHighpass[0], kSfHighpass[1], kSfHighpass[2], kSfHighpass[3], kSfHighpass[4], shelved, h0, h1);
      acc += y * y;
      if (Masked && on[t][column]) masked_acc += y * y;
      if (++in_chunk == kSfHop) {
        if (valid && chunk < n_chunks) energy[(int64_t)s * n_chunks + chunk] = acc;
        if (Masked && valid && chunk < n_chunks) masked_energy[(int64_t)s * n_chunks + chunk] = masked_acc;
        acc = 0.0;
        masked_acc = 0.0;
        in_chunk = 0;
        ++chunk;
      }
    }
    __syncthreads();
  }
  if (in_chunk > 0 && valid && chunk < n_chunks) {  // the partial tail
    energy[(int64_t)s * n_chunks + chunk] = acc;
    if (Masked) masked_energy[(int64_t)s * n_chunks + chunk] = masked_acc;
  }
  if (Masked && valid) { state[4 * s] = a0; state[4 * s + 1] = a1; state[4 * s + 2] = h0; state[4 * s + 3] = h1; }
}

// scipy.signal.resample_poly of the captures and of their activity masks to 48 kHz, the chunks chunk0 .. chunk0 + gridDim.x of
// every stream into a scratch row of `row` samples: a workgroup takes one chunk of 960 outputs of one stream, stages the inputs they reach (at most kSfResampleSpan, checked by the launcher) in LDS as f64 -- the
// samples, and the mask made from the frame flags: sample j is active when frame j / hop or the one before it is -- and every
// thread sums its outputs' products over the taps of their phase, the oldest input first, multiplied and added apart.  The phase
// table (up x taps doubles: 27 KB at 160 / 147, 54 KB at 320 / 147) is read from global memory: every workgroup reads the same
// rows, so it stays in L2, and LDS is left to the inputs.  Leaves y[s][o], mask bytes (resampled mask >= 0.5) and their count.
__global__ void __launch_bounds__(kSfResampleThreads) sf_resample_kernel(const float *__restrict__ audio, int64_t stride, int64_t n,
                                                                          const uint8_t *__restrict__ active, int32_t n_frames, int32_t hop,
                                                                          SfResamplePlan plan, const double *__restrict__ table, int64_t n48,
                                                                          int32_t n_chunks, int32_t chunk0, int64_t row,
                                                                          double *__restrict__ y, uint8_t *__restrict__ mask,
                                                                          int32_t *__restrict__ count) {
  __shared__ double xs[kSfResampleSpan], ms[kSfResampleSpan];
  __shared__ int32_t wave_count[kSfResampleThreads / 64];
  const int s = blockIdx.y, tid = threadIdx.x;
  const int64_t base = (int64_t)chunk0 * kSfHop, o0 = base + (int64_t)blockIdx.x * kSfHop, o1 = o0 + kSfHop < n48 ? o0 + kSfHop : n48;
  const int64_t first = ((o0 + plan.rem) * plan.down) / plan.up - (plan.taps - 1), last = ((o1 - 1 + plan.rem) * plan.down) / plan.up;
  const int span = (int)(last - first + 1);  // <= kSfResampleSpan
  const uint8_t *flags = active + (int64_t)s * n_frames;
  for (int i = tid; i < span; i += kSfResampleThreads) {
    const int64_t j = first + i;
    double v = 0.0, m = 0.0;
    if (j >= 0 && j < n) {
      const int64_t f = j / hop;
      v = (double)audio[(int64_t)s * stride + j];
      m = ((f < n_frames && flags[f]) || (f >= 1 && f - 1 < n_frames && flags[f - 1])) ? 1.0 : 0.0;
    }
    xs[i] = v;
    ms[i] = m;
  }
  __syncthreads();
  int32_t mine = 0;
  for (int64_t o = o0 + tid; o < o1; o += kSfResampleThreads) {
    const int64_t t = (o + plan.rem) * plan.down, xi = t / plan.up;
    const double *phase = table + (int64_t)(t % plan.up) * plan.taps;
    double acc = 0.0, macc = 0.0;
    for (int m = plan.taps - 1; m >= 0; --m) {
      const int64_t j = xi - m;
      if (j >= 0 && j < n) {
        const double h = phase[m];
        acc += xs[j - first] * h;
        macc += ms[j - first] * h;
      }
    }
    const uint8_t bit = macc >= 0.5;
    y[(int64_t)s * row + (o - base)] = acc;
    mask[(int64_t)s * row + (o - base)] = bit;
    mine += bit;
  }
  for (int off = 32; off >= 1; off >>= 1) mine += __shfl_xor(mine, off, 64);
  if ((tid & 63) == 0) wave_count[tid >> 6] = mine;
  __syncthreads();
  if (tid == 0) {
    int32_t total = 0;
    for (int w = 0; w < kSfResampleThreads / 64; ++w) total += wave_count[w];
    count[(int64_t)s * n_chunks + chunk0 + blockIdx.x] = total;
  }
}

// P: bins a thread, (hop + kSfThreads) / kSfThreads of them at the most: 4 up to a hop of 960, 8 up to kSfMaxHop.  The
// half-length transform lives in dynamic LDS, 16 bytes a point: 15 KB at 48 kHz, 30 KB at 96 kHz.
template <int P>
__global__ void __launch_bounds__(kSfThreads) sf_frame_kernel(const float *__restrict__ speech, int64_t speech_stride,
                                                               const float *__restrict__ noise, int64_t noise_stride,
                                                               const SfFrameItem *__restrict__ items, int32_t hop, NrPlan plan, SfBandTable bands,
                                                               const double *__restrict__ window, const double2 *__restrict__ tw,
                                                               double *__restrict__ band, double *__restrict__ sib_mid,
                                                               int32_t *__restrict__ sib_arg, double *__restrict__ sib_rows,
                                                               double *__restrict__ noise_band) {
  extern __shared__ double2 buf[];  // [hop] the half-length transform; the power row as doubles once it has been read
  __shared__ double wave_total[kSfThreads / 64];
  const SfFrameItem it = items[blockIdx.x];
  constexpr int T = kSfThreads;
  const int M = hop, frame = 2 * hop, tid = threadIdx.x;
  const float *x = (it.source ? speech + (int64_t)it.stream * speech_stride : noise + (int64_t)it.stream * noise_stride) + (int64_t)it.chunk * hop;
  double sum = 0.0;  // np.mean(frame), :280: strided partial sums, an xor tree per wave, the waves in order
  for (int i = tid; i < frame; i += T) sum += (double)x[i];
  sum = sf_wave_sum(sum);
  if ((tid & 63) == 0) wave_total[tid >> 6] = sum;
  __syncthreads();
  const double mean = (((wave_total[0] + wave_total[1]) + wave_total[2]) + wave_total[3]) / (double)frame;
  for (int m = tid; m < M; m += T)
    buf[m] = make_double2(((double)x[2 * m] - mean) * window[2 * m], ((double)x[2 * m + 1] - mean) * window[2 * m + 1]);
  __syncthreads();
  nr_transform(buf, M, plan, tw);
  double p[P];  // bins tid, tid + T, ...: M + 1 of them in all
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int k = tid + j * T;
    p[j] = k <= M ? nr_real_bin_power(buf, k, M, plan, tw) + 1e-18 : 0.0;
  }
  __syncthreads();  // every read of the transform is done: the buffer now takes the row
  double *pw = reinterpret_cast<double *>(buf);
#pragma unroll
  for (int j = 0; j < P; ++j) {
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

hipError_t launch_sf_frame_power(const float *audio, int64_t stride, int32_t n_streams, int32_t n_frames, int32_t frame, int32_t hop,
                                 double *power, hipStream_t stream) {
  const int64_t total = (int64_t)n_streams * n_frames, per = kSfThreads / 64;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(sf_frame_power_kernel, dim3((unsigned)((total + per - 1) / per)), dim3(kSfThreads), 0, stream, audio, stride, total,
                     n_frames, frame, hop, power);
  return hipGetLastError();
}

hipError_t launch_sf_kweight(const float *audio, int64_t stride, int64_t n, int32_t n_streams, int32_t n_chunks, double *energy,
                             hipStream_t stream) {
  if (n_streams <= 0 || n <= 0) return hipSuccess;
  int per = kSfLanes;  // the recurrence is latency-bound: spread a small batch over the compute units before filling the lanes
  while (per > kSfMinStreamsPerGroup && (n_streams + per - 1) / per < kSfComputeUnits) per /= 2;
  hipLaunchKernelGGL((sf_kweight_kernel<float, false>), dim3((unsigned)((n_streams + per - 1) / per)), dim3(kSfLanes), 0, stream, audio,
                     stride, n, n_streams, n_chunks, per, energy, (const uint8_t *)nullptr, (double *)nullptr, (double *)nullptr, 0);
  return hipGetLastError();
}

hipError_t launch_sf_kweight_resampled(const double *signal, const uint8_t *mask, int64_t row, int64_t n, int32_t n_streams, int32_t n_chunks,
                                       int32_t chunk0, double *state, double *energy, double *masked_energy, hipStream_t stream) {
  if (n_streams <= 0 || n <= 0) return hipSuccess;
  if (n > row || chunk0 < 0 || chunk0 + (n + kSfHop - 1) / kSfHop > n_chunks) return hipErrorInvalidValue;
  int per = kSfLanes;
  while (per > kSfMinStreamsPerGroup && (n_streams + per - 1) / per < kSfComputeUnits) per /= 2;
  hipLaunchKernelGGL((sf_kweight_kernel<double, true>), dim3((unsigned)((n_streams + per - 1) / per)), dim3(kSfLanes), 0, stream, signal,
                     row, n, n_streams, n_chunks, per, energy, mask, masked_energy, state, chunk0);
  return hipGetLastError();
}

hipError_t launch_sf_resample(const float *audio, int64_t stride, int64_t n, int32_t n_streams, const uint8_t *active, int32_t n_frames,
                              int32_t hop, const SfResamplePlan &plan, const double *table, int64_t n48, int32_t chunk0, int32_t chunks,
                              int64_t row, double *signal, uint8_t *mask, int32_t *count, hipStream_t stream) {
  if (n_streams <= 0 || n48 <= 0 || chunks <= 0) return hipSuccess;
  const int32_t n_chunks = (int32_t)((n48 + kSfHop - 1) / kSfHop);
  if (plan.up <= 0 || plan.down <= 0 || plan.taps <= 0 || sf_resample_span(plan) > kSfResampleSpan || chunk0 < 0 ||
      chunk0 + chunks > n_chunks || row < (int64_t)chunks * kSfHop)
    return hipErrorInvalidValue;
  for (int32_t s0 = 0; s0 < n_streams; s0 += 65535) {  // gridDim.y holds 65535 streams
    const int32_t S = n_streams - s0 < 65535 ? n_streams - s0 : 65535;
    hipLaunchKernelGGL(sf_resample_kernel, dim3((unsigned)chunks, (unsigned)S), dim3(kSfResampleThreads), 0, stream,
                       audio + (int64_t)s0 * stride, stride, n, active + (int64_t)s0 * n_frames, n_frames, hop, plan, table, n48, n_chunks,
                       chunk0, row, signal + (int64_t)s0 * row, mask + (int64_t)s0 * row, count + (int64_t)s0 * n_chunks);
  }
  return hipGetLastError();
}

hipError_t launch_sf_frames(const float *speech, int64_t speech_stride, const float *noise, int64_t noise_stride, const SfFrameItem *items,
                            int32_t n_items, int32_t hop, const NrPlan &plan, const SfBandTable &bands, const double *window, const double *twiddles,
                            double *band, double *sib_mid, int32_t *sib_arg, double *sib_rows, double *noise_band, hipStream_t stream) {
  if (n_items <= 0) return hipSuccess;
  if (hop <= 0 || hop > kSfMaxHop) return hipErrorInvalidValue;
  const size_t lds = sizeof(double2) * (size_t)hop;
  if ((hop + kSfThreads) / kSfThreads <= 4)
    hipLaunchKernelGGL(sf_frame_kernel<4>, dim3((unsigned)n_items), dim3(kSfThreads), lds, stream, speech, speech_stride, noise, noise_stride,
                       items, hop, plan, bands, window, (const double2 *)twiddles, band, sib_mid, sib_arg, sib_rows, noise_band);
  else
    hipLaunchKernelGGL(sf_frame_kernel<8>, dim3((unsigned)n_items), dim3(kSfThreads), lds, stream, speech, speech_stride, noise, noise_stride,
                       items, hop, plan, bands, window, (const double2 *)twiddles, band, sib_mid, sib_arg, sib_rows, noise_band);
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
