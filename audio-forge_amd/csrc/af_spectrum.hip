// af_spectrum.hip -- kernels of the batched voice spectrum measurement (python/mic_eq/analysis/spectrum.py): chunk sums for the
// frame energies and means, Hamming-windowed real FFTs in LDS for the window spectra and the Welch spectrum, masked column
// medians, and the perceptual fractional-octave smoothing.  All arithmetic is f64 and unfused (-ffp-contract=off); window,
// twiddles and band tables come from the host.  tests/ref/voice_spectrum_ref.c restates every operation in the same order.
#include <hip/hip_runtime.h>

#include "af_spectrum_host.hpp"

namespace af {
namespace {

constexpr int kVsThreads = 256;

// One wave per hop-sized chunk: lane l sums samples l, l + 64, ... in order, then an xor tree leaves the same total in every lane.
__global__ void __launch_bounds__(kVsThreads) vs_chunk_sums_kernel(const float *__restrict__ audio, int64_t stride, int64_t total,
                                                                    int32_t n_chunks, int32_t hop, double *__restrict__ sums) {
  const int lane = threadIdx.x & 63;
  const int64_t id = (int64_t)blockIdx.x * (kVsThreads / 64) + (threadIdx.x >> 6);
  if (id >= total) return;  // whole waves leave together
  const int64_t s = id / n_chunks, c = id % n_chunks;
  const float *x = audio + s * stride + c * hop;
  double a = 0.0, q = 0.0;
  for (int i = lane; i < hop; i += 64) {
    const double v = (double)x[i];
    a += v;
    q += v * v;
  }
  for (int off = 32; off >= 1; off >>= 1) {
    a += __shfl_xor(a, off, 64);
    q += __shfl_xor(q, off, 64);
  }
  if (lane == 0) {
    sums[id * 2] = a;
    sums[id * 2 + 1] = q;
  }
}

// (x - mean) * w of the frame made of chunks ca | cb as M = N/2 complex points, then a radix-2 decimation-in-frequency
// transform in place: Z[k] ends at buf[bitrev(k)].  Ends behind a barrier.
__device__ void vs_segment_fft(double2 *buf, const float *__restrict__ ca, const float *__restrict__ cb, double mean, int M,
                               const double *__restrict__ w, const double2 *__restrict__ tw) {
  const int tid = threadIdx.x, T = blockDim.x;
  for (int m = tid; m < M; m += T) {
    const int i = 2 * m;
    const float *src = i < M ? ca + i : cb + (i - M);  // M is even: both samples lie in one chunk
    buf[m] = make_double2(((double)src[0] - mean) * w[i], ((double)src[1] - mean) * w[i + 1]);
  }
  __syncthreads();
  for (int half = M / 2; half >= 1; half >>= 1) {
    const int step = M / (2 * half);
    for (int j = tid; j < M / 2; j += T) {
      const int pos = j % half, i0 = (j / half) * 2 * half + pos, i1 = i0 + half;
      const double2 a = buf[i0], b = buf[i1], t = tw[2 * pos * step];  // exp(-2 pi i pos step / M)
      const double dr = a.x - b.x, di = a.y - b.y;
      buf[i0] = make_double2(a.x + b.x, a.y + b.y);
      buf[i1] = make_double2(dr * t.x - di * t.y, dr * t.y + di * t.x);
    }
    __syncthreads();
  }
}

// |X[k]|^2 of the real transform from the half-length complex one, k = 0 .. M
__device__ double vs_bin_power(const double2 *buf, int k, int M, int bits, const double2 *__restrict__ tw) {
  const unsigned ia = __brev((unsigned)(k % M)) >> (32 - bits), ib = __brev((unsigned)((M - k) % M)) >> (32 - bits);
  const double2 a = buf[ia], b = buf[ib], t = tw[k];
  const double er = 0.5 * (a.x + b.x), ei = 0.5 * (a.y - b.y);
  const double orr = 0.5 * (a.y + b.y), oi = -0.5 * (a.x - b.x);
  const double xr = er + (orr * t.x - oi * t.y), xi = ei + (orr * t.y + oi * t.x);
  return xr * xr + xi * xi;
}

__device__ int vs_log2(int M) {
  int bits = 0;
  while ((1 << bits) < M) ++bits;
  return bits;
}

__global__ void __launch_bounds__(kVsThreads) vs_window_kernel(const float *__restrict__ audio, int64_t stride,
                                                                const double *__restrict__ sums, int32_t n_chunks,
                                                                const float *__restrict__ noise, int64_t noise_stride,
                                                                const double *__restrict__ noise_sums, int32_t noise_chunks,
                                                                const VsWindowItem *__restrict__ items, int32_t nperseg,
                                                                const double *__restrict__ window, const double2 *__restrict__ tw,
                                                                double sumw2, double *__restrict__ db, double *__restrict__ linear) {
  extern __shared__ double2 vs_buf[];
  const VsWindowItem it = items[blockIdx.x];
  const int M = nperseg / 2, bits = vs_log2(M);
  const float *x = it.source ? noise + (int64_t)it.stream * noise_stride : audio + (int64_t)it.stream * stride;
  const double *sm = it.source ? noise_sums + ((int64_t)it.stream * noise_chunks + it.chunk) * 2
                               : sums + ((int64_t)it.stream * n_chunks + it.chunk) * 2;
  const double mean = (sm[0] + sm[2]) / (double)nperseg;
  vs_segment_fft(vs_buf, x + (int64_t)it.chunk * M, x + (int64_t)(it.chunk + 1) * M, mean, M, window, tw);
  const int64_t base = (int64_t)it.row * (M + 1);
  for (int k = threadIdx.x; k <= M; k += blockDim.x) {
    const double psd = vs_bin_power(vs_buf, k, M, bits, tw) / sumw2;
    linear[base + k] = psd;
    if (db) db[base + k] = 10.0 * log10(psd + 1e-12);
  }
}

__global__ void __launch_bounds__(kVsThreads) vs_welch_kernel(const float *__restrict__ audio, int64_t stride,
                                                               const double *__restrict__ sums, int32_t n_chunks,
                                                               const int32_t *__restrict__ chunks, const int32_t *__restrict__ offset,
                                                               int32_t nperseg, const double *__restrict__ window,
                                                               const double2 *__restrict__ tw, double scale, double *__restrict__ sum,
                                                               double *__restrict__ db) {
  extern __shared__ double2 vs_buf[];
  const int s = blockIdx.x, M = nperseg / 2, bits = vs_log2(M);
  const int32_t *c = chunks + offset[s];
  const int nseg = offset[s + 1] - offset[s] - 1;
  const float *x = audio + (int64_t)s * stride;
  const double *sm = sums + (int64_t)s * n_chunks * 2;
  double *acc = sum + (int64_t)s * (M + 1);
  for (int j = 0; j < nseg; ++j) {  // segment order, every bin owned by one thread: no atomics, the same bits every run
    const int a = c[j], b = c[j + 1];
    const double mean = (sm[2 * a] + sm[2 * b]) / (double)nperseg;
    vs_segment_fft(vs_buf, x + (int64_t)a * M, x + (int64_t)b * M, mean, M, window, tw);
    for (int k = threadIdx.x; k <= M; k += blockDim.x) {
      const double p = vs_bin_power(vs_buf, k, M, bits, tw);
      acc[k] = j == 0 ? p : acc[k] + p;
    }
    __syncthreads();  // the next segment overwrites the buffer
  }
  for (int k = threadIdx.x; k <= M; k += blockDim.x) {  // signal.welch: density scaling, one-sided doubling, mean over segments
    double v = acc[k] * scale;
    if (k > 0 && k < M) v = v * 2.0;
    v = v / (double)nseg;
    db[(int64_t)s * (M + 1) + k] = 10.0 * log10(v + 1e-12);
  }
}

// The k-th smallest (0-based) of col[0], col[stride], ... (n finite values): narrow an open interval around it, one pass per
// pivot; the next pivot is the in-range value with the smallest hash of its index.  *below / *equal: the pivot's counts.
__device__ double vs_select(const double *__restrict__ col, int64_t stride, int n, int k, int *below, int *equal) {
  double lo = -INFINITY, hi = INFINITY, pivot = col[(int64_t)(n / 2) * stride];
  for (unsigned pass = 1; pass <= (unsigned)n + 1u; ++pass) {  // every pass removes its pivot from the interval: at most n passes
    int cl = 0, ce = 0;
    unsigned best_l = 0xffffffffu, best_h = 0xffffffffu;
    double cand_l = pivot, cand_h = pivot;
    for (int i = 0; i < n; ++i) {
      const double v = col[(int64_t)i * stride];
      cl += v < pivot;
      ce += v == pivot;
      unsigned h = ((unsigned)i + 1u) * 2654435761u ^ pass * 0x9e3779b9u;
      h ^= h >> 15;
      h *= 0x85ebca6bu;
      h ^= h >> 13;
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

__global__ void __launch_bounds__(kVsThreads) vs_median_kernel(const double *__restrict__ rows, const VsMedianJob *__restrict__ jobs,
                                                                int32_t bins, double *__restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= bins) return;
  const VsMedianJob job = jobs[blockIdx.y];
  const double *col = rows + (int64_t)job.row0 * bins + k;
  const int n = job.count;
  int below, equal;
  const double a = vs_select(col, bins, n, (n - 1) / 2, &below, &equal);
  double b = a;
  if (!(n & 1) && n / 2 >= below + equal) {  // an even count: the upper middle is the smallest value above a
    b = INFINITY;
    for (int i = 0; i < n; ++i) {
      const double v = col[(int64_t)i * bins];
      if (v > a && v < b) b = v;
    }
  }
  out[((int64_t)job.out * 2) * bins + k] = a;
  out[((int64_t)job.out * 2 + 1) * bins + k] = b;
}

// smooth_spectrum_perceptual "balanced" of one window spectrum per workgroup (spectrum.py:892-967)
__global__ void __launch_bounds__(kVsThreads) vs_smooth_kernel(const double *__restrict__ rows, const int32_t *__restrict__ row_index,
                                                                int32_t bins, const int32_t *__restrict__ n_bands,
                                                                const double *__restrict__ centre, const int32_t *__restrict__ first,
                                                                const int32_t *__restrict__ last, const int32_t *__restrict__ bin_pass,
                                                                const int32_t *__restrict__ bin_index, const double *__restrict__ freqs,
                                                                double *__restrict__ out) {
  extern __shared__ double vs_pw[];  // [bins] linear power
  __shared__ double y[kVsSmoothPasses * kVsMaxBands];
  const double *row = rows + (int64_t)row_index[blockIdx.x] * bins;
  for (int k = threadIdx.x; k < bins; k += blockDim.x) vs_pw[k] = pow(10.0, row[k] / 10.0);
  __syncthreads();
  for (int t = threadIdx.x; t < kVsSmoothPasses * kVsMaxBands; t += blockDim.x) {
    const int p = t / kVsMaxBands, b = t % kVsMaxBands;
    if (b >= n_bands[p]) continue;
    const int f0 = first[t], f1 = last[t];
    double s = 0.0;
    for (int k = f0; k <= f1; ++k) s += vs_pw[k];
    y[t] = 10.0 * log10(s / (double)(f1 - f0 + 1));
  }
  __syncthreads();
  for (int k = threadIdx.x; k < bins; k += blockDim.x) {
    const int p = bin_pass[k], idx = bin_index[k], n = n_bands[p];
    const double *yp = y + p * kVsMaxBands, *xc = centre + p * kVsMaxBands;
    double v;
    if (idx == -3) v = row[k];
    else if (idx == -1) v = yp[0];
    else if (idx == -2) v = yp[n - 1];
    else {  // np.interp
      const double slope = (yp[idx + 1] - yp[idx]) / (xc[idx + 1] - xc[idx]);
      v = slope * (freqs[k] - xc[idx]) + yp[idx];
    }
    out[(int64_t)blockIdx.x * bins + k] = v;
  }
}

int vs_threads(int nperseg) { return nperseg / 4 < kVsThreads ? nperseg / 4 : kVsThreads; }  // one butterfly per thread and stage at least

}  // namespace

hipError_t launch_vs_chunk_sums(const float *audio, int64_t stride, int32_t n_streams, int32_t n_chunks, int32_t hop, double *sums,
                                hipStream_t stream) {
  const int64_t total = (int64_t)n_streams * n_chunks;
  if (total <= 0) return hipSuccess;
  const int64_t blocks = (total + kVsThreads / 64 - 1) / (kVsThreads / 64);
  hipLaunchKernelGGL(vs_chunk_sums_kernel, dim3((unsigned)blocks), dim3(kVsThreads), 0, stream, audio, stride, total, n_chunks, hop, sums);
  return hipGetLastError();
}

hipError_t launch_vs_window_spectra(const float *audio, int64_t stride, const double *sums, int32_t n_chunks, const float *noise,
                                    int64_t noise_stride, const double *noise_sums, int32_t noise_chunks, const VsWindowItem *items,
                                    int32_t n_items, int32_t nperseg, const double *window, const double *twiddles, double sumw2,
                                    double *db, double *linear, hipStream_t stream) {
  if (n_items <= 0) return hipSuccess;
  const size_t lds = sizeof(double2) * (size_t)(nperseg / 2);
  hipLaunchKernelGGL(vs_window_kernel, dim3((unsigned)n_items), dim3(vs_threads(nperseg)), lds, stream, audio, stride, sums, n_chunks,
                     noise, noise_stride, noise_sums, noise_chunks, items, nperseg, window, (const double2 *)twiddles, sumw2, db, linear);
  return hipGetLastError();
}

hipError_t launch_vs_welch(const float *audio, int64_t stride, const double *sums, int32_t n_chunks, const int32_t *chunks,
                           const int32_t *offset, int32_t n_streams, int32_t nperseg, const double *window, const double *twiddles,
                           double scale, double *sum, double *db, hipStream_t stream) {
  if (n_streams <= 0) return hipSuccess;
  const size_t lds = sizeof(double2) * (size_t)(nperseg / 2);
  hipLaunchKernelGGL(vs_welch_kernel, dim3((unsigned)n_streams), dim3(vs_threads(nperseg)), lds, stream, audio, stride, sums, n_chunks,
                     chunks, offset, nperseg, window, (const double2 *)twiddles, scale, sum, db);
  return hipGetLastError();
}

hipError_t launch_vs_median(const double *rows, const VsMedianJob *jobs, int32_t n_jobs, int32_t bins, double *out, hipStream_t stream) {
  if (n_jobs <= 0) return hipSuccess;
  hipLaunchKernelGGL(vs_median_kernel, dim3((unsigned)((bins + kVsThreads - 1) / kVsThreads), (unsigned)n_jobs), dim3(kVsThreads), 0,
                     stream, rows, jobs, bins, out);
  return hipGetLastError();
}

hipError_t launch_vs_smooth(const double *rows, const int32_t *row_index, int32_t n_rows, int32_t bins, const int32_t *n_bands,
                            const double *centre, const int32_t *first, const int32_t *last, const int32_t *bin_pass,
                            const int32_t *bin_index, const double *freqs, double *out, hipStream_t stream) {
  if (n_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(vs_smooth_kernel, dim3((unsigned)n_rows), dim3(kVsThreads), sizeof(double) * (size_t)bins, stream, rows, row_index,
                     bins, n_bands, centre, first, last, bin_pass, bin_index, freqs, out);
  return hipGetLastError();
}

}  // namespace af
