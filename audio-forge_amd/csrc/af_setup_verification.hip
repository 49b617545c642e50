// af_setup_verification.hip -- the kernels of the second-passage measurements (voice_setup.py:1446-1679), f64 throughout.
//   sv_shape_kernel : one workgroup of 256 per stream.  _shape_error_db of the before and the after spectrum against the adaptive
//                     house curve, the repeatability delta, the four band medians of the spectral SNR.  Every sum is the "svm sum"
//                     of af_setup_verification_math.h (lane t adds terms t, t + 256, ...; then a halving tree), every median an
//                     exact selection from a bitonic sort in LDS (padded with +inf; a NaN anywhere makes the median NaN, np.median).
//   sv_levels_kernel: one workgroup of 256 per (stream, signal).  NumPy's sum of squares: a wave takes a buffer of 8192 samples,
//                     its lane l the node that the bits of l, most significant first, lead to from the buffer's root (left = 0:
//                     a block of at most 128 samples, or a node of at most 135 that splits once more), sums it with the
//                     restatement's own recursion, and the six levels above are
//                     added in LDS, left + right, as the recursion does; thread 0 adds the buffers in order.  Peak and flags
//                     are order-free and read the signal with unit stride across lanes.
// LDS per workgroup: 2 KiB + 8 B x sort capacity (at most 34 KiB), so several workgroups share a CU; nothing here is sized by it.
#include <hip/hip_runtime.h>

#define SVM_FN __host__ __device__ static inline
#include "af_setup_verification_host.hpp"
#include "af_setup_verification_math.h"

namespace af {
namespace {

constexpr int T = kSvThreads;

// the svm sum of term(i), i < n: every thread returns it
template <class F>
__device__ double sv_block_sum(double *red, int n, F term) {
  const int t = (int)threadIdx.x;
  double p = 0.0;
  for (int i = t; i < n; i += T) p += term(i);
  red[t] = p;
  __syncthreads();
  for (int s = T / 2; s >= 1; s /= 2) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  const double total = red[0];
  __syncthreads();
  return total;
}

// np.median of value(i), i < n (1 <= n <= capacity, a power of two): every thread returns it
template <class F>
__device__ double sv_block_median(double *sorted, int capacity, int n, F value) {
  const int t = (int)threadIdx.x;
  int nan_here = 0;
  for (int i = t; i < capacity; i += T) {
    double v = INFINITY;
    if (i < n) {
      v = value(i);
      if (v != v) { nan_here = 1; v = INFINITY; }
    }
    sorted[i] = v;
  }
  const int any_nan = __syncthreads_or(nan_here);
  for (int k = 2; k <= capacity; k *= 2)
    for (int j = k / 2; j >= 1; j /= 2) {
      for (int i = t; i < capacity; i += T) {
        const int partner = i ^ j;
        if (partner > i) {
          const double a = sorted[i], b = sorted[partner];
          const bool ascending = (i & k) == 0;
          if (ascending ? a > b : a < b) { sorted[i] = b; sorted[partner] = a; }
        }
      }
      __syncthreads();
    }
  const double median = n % 2 ? sorted[n / 2] : (sorted[n / 2 - 1] + sorted[n / 2]) / 2.0;
  __syncthreads();
  return any_nan ? (double)NAN : median;
}

// _shape_error_db of one spectrum's masked bins m[0..n) at f[0..n); n >= SVM_MIN_BINS
__device__ double sv_shape_error(double *red, double *sorted, const SvGrid &g, const double *f, const double *m, int preset,
                                 svm_offset_scalars *scalars) {
  const int n = g.count;
  auto band_mean = [&](double low, double high, int count) {
    if (!count) return sv_block_sum(red, n, [&](int i) { return m[i]; }) / (double)n;
    return sv_block_sum(red, n, [&](int i) { return f[i] >= low && f[i] <= high ? m[i] : 0.0; }) / (double)count;
  };
  const double body = band_mean(180.0, 800.0, g.body_count), presence = band_mean(1200.0, 3500.0, g.presence_count);
  const double sibilance = band_mean(5500.0, 8500.0, g.sibilance_count);
  double tilt = 0.0;
  if (g.voice_count >= 2) {
    auto voice = [&](int i) { return f[i] >= 100.0 && f[i] <= 8000.0; };
    const double mean_x = sv_block_sum(red, n, [&](int i) { return voice(i) ? svm_log10_frequency(f[i]) : 0.0; }) / (double)g.voice_count;
    const double mean_y = sv_block_sum(red, n, [&](int i) { return voice(i) ? m[i] : 0.0; }) / (double)g.voice_count;
    const double denom = sv_block_sum(red, n, [&](int i) {
      const double xc = svm_log10_frequency(f[i]) - mean_x;
      return voice(i) ? xc * xc : 0.0;
    });
    const double dot = sv_block_sum(red, n, [&](int i) {
      const double xc = svm_log10_frequency(f[i]) - mean_x;
      return voice(i) ? xc * (m[i] - mean_y) : 0.0;
    });
    if (denom > 0.0) tilt = dot / denom;
  }
  svm_offset_rules(body, presence, sibilance, tilt, scalars);
  auto target = [&](int i) { return svm_catalog_curve(preset, f[i]) + svm_offset_at(preset, scalars, f[i]); };
  const double m0 = sv_block_median(sorted, g.sort_capacity, n, [&](int i) { return m[i]; });
  const double t0 = sv_block_median(sorted, g.sort_capacity, n, target);
  const double sum = sv_block_sum(red, n, [&](int i) {
    const double d = (m[i] - m0) - (target(i) - t0);
    return d * d;
  });
  return sqrt(sum / (double)n);
}

__global__ __launch_bounds__(T) void sv_shape_kernel(SvGrid g, const double *__restrict__ freqs, const double *__restrict__ original_db,
                                                     const double *__restrict__ before_db, const double *__restrict__ after_db,
                                                     int64_t spectrum_stride, const double *__restrict__ after_snr_db, int64_t snr_stride,
                                                     const int32_t *__restrict__ preset_ids, af_setup_verification_row *__restrict__ rows) {
  extern __shared__ __attribute__((aligned(16))) double sv_lds[];
  double *red = sv_lds, *sorted = sv_lds + T;
  const int stream = (int)blockIdx.x, n = g.count;
  const int preset = preset_ids[stream];
  const double *f = freqs + g.first;
  const double *original = original_db + (int64_t)stream * spectrum_stride + g.first;
  const double *before = before_db + (int64_t)stream * spectrum_stride + g.first;
  const double *after = after_db + (int64_t)stream * spectrum_stride + g.first;
  svm_offset_scalars scalars_before, scalars_after;
  double error_before = INFINITY, error_after = INFINITY, delta = NAN, band[4] = {0.0, 0.0, 0.0, 0.0};
  int present[4] = {0, 0, 0, 0};
  memset(&scalars_before, 0, sizeof scalars_before);
  memset(&scalars_after, 0, sizeof scalars_after);

  if (n >= SVM_MIN_BINS) {
    error_before = sv_shape_error(red, sorted, g, f, before, preset, &scalars_before);
    error_after = sv_shape_error(red, sorted, g, f, after, preset, &scalars_after);
  }
  if (n > 0) {  // :1562-1575 on the shared grid
    const double d0 = sv_block_median(sorted, g.sort_capacity, n, [&](int i) { return before[i] - original[i]; });
    const double sum = sv_block_sum(red, n, [&](int i) {
      const double d = (before[i] - original[i]) - d0;
      return d * d;
    });
    delta = sqrt(sum / (double)n);
  }
  if (after_snr_db) {
    const double *snr = after_snr_db + (int64_t)stream * snr_stride;
    for (int b = 0; b < 4; ++b) {
      if (!g.band_count[b]) continue;
      present[b] = 1;
      band[b] = sv_block_median(sorted, g.sort_capacity, g.band_count[b], [&](int i) { return snr[g.band_first[b] + i]; });
    }
  }
  if (threadIdx.x == 0) {
    af_setup_verification_row *row = rows + stream;
    const double *sb = &scalars_before.body_db, *sa = &scalars_after.body_db;  // the five reported scalars lead the struct
    row->masked_bins = n;
    row->snr_available = after_snr_db != nullptr;
    row->reserved = 0;
    row->spectral_target_error_before_db = error_before;
    row->spectral_target_error_after_db = error_after;
    row->shape_delta_db = delta;
    for (int b = 0; b < 4; ++b) {
      row->band_present[b] = present[b];
      row->band_snr_db[b] = band[b];
    }
    for (int k = 0; k < 5; ++k) {
      row->offsets_before[k] = sb[k];
      row->offsets_after[k] = sa[k];
    }
  }
}

__global__ __launch_bounds__(T) void sv_levels_kernel(SvAudio audio, af_setup_verification_row *__restrict__ rows) {
  __shared__ double red[T];
  __shared__ int here[T];
  const int t = (int)threadIdx.x, stream = (int)blockIdx.x, signal = (int)blockIdx.y;
  af_setup_verification_row *row = rows + stream;
  if (!audio.samples[signal]) {  // uniform over the workgroup
    if (t == 0) {
      row->sum_squares[signal] = 0.0;
      row->peak[signal] = 0.0;
      row->rms_db[signal] = -120.0;
      row->non_finite[signal] = row->clipped_0999[signal] = row->clipped_1[signal] = 0;
    }
    return;
  }
  const int64_t n = audio.lengths[signal] ? audio.lengths[signal][stream] : audio.length[signal];
  const float *x = audio.samples[signal] + (int64_t)stream * audio.stride[signal];

  // NumPy's order: buffers of 8192 samples, one per wave and pass, added to the total in order by thread 0.  Inside a buffer
  // lane l takes the node that the six bits of l lead to (left = 0); a block reached early lives where the remaining bits are zero.
  // Halves are cut at multiples of eight, so the right-hand nodes of a short last buffer grow: after six halvings a node may
  // still hold more than 128 samples (135 of 8191), and the lane finishes it with the restatement's own recursion.
  const int wave = t / 64, lane = t % 64;
  double sum_squares = 0.0;  // thread 0's
  for (int64_t base = 0; base < n; base += (int64_t)(T / 64) * SVM_PAIRWISE_BUFFER) {
    const int64_t start = base + (int64_t)wave * SVM_PAIRWISE_BUFFER;
    int64_t lo = 0, len = n - start < SVM_PAIRWISE_BUFFER ? n - start : SVM_PAIRWISE_BUFFER;
    int present = len > 0;
    for (int b = 5; b >= 0; --b) {
      const int bit = (lane >> b) & 1;
      if (len > SVM_PAIRWISE_BLOCK) {
        const int64_t half = svm_pairwise_left(len);
        if (bit) { lo += half; len -= half; } else len = half;
      } else if (bit) {
        present = 0;
      }
    }
    red[t] = present ? svm_pairwise_sum_squares(x + start + lo, len) : 0.0;
    here[t] = present;
    __syncthreads();
    for (int s = 1; s < 64; s *= 2) {
      if (lane % (2 * s) == 0 && here[t + s]) red[t] = red[t] + red[t + s];
      __syncthreads();
    }
    if (t == 0)
      for (int w = 0; w < T / 64; ++w)
        if (here[64 * w]) sum_squares += red[64 * w];
    __syncthreads();
  }

  double top = 0.0;
  int bad = 0;
  for (int64_t i = t; i < n; i += T) {
    const float v = x[i];
    const double a = fabs((double)v);
    bad |= !isfinite(v);
    if (a > top) top = a;
  }
  red[t] = top;
  const int any_bad = __syncthreads_or(bad);
  for (int s = T / 2; s >= 1; s /= 2) {
    if (t < s && red[t + s] > red[t]) red[t] = red[t + s];
    __syncthreads();
  }
  if (t == 0) {
    const double peak = red[0];
    row->sum_squares[signal] = sum_squares;
    row->peak[signal] = peak;
    row->rms_db[signal] = svm_rms_db(sum_squares, n);
    row->non_finite[signal] = any_bad;
    row->clipped_0999[signal] = peak >= 0.999;
    row->clipped_1[signal] = peak >= 1.0;
  }
}

}  // namespace

hipError_t launch_setup_verification_shape(const SvGrid &grid, const double *freqs, const double *original_db, const double *before_db,
                                           const double *after_db, int64_t spectrum_stride, const double *after_snr_db,
                                           int64_t snr_stride, const int32_t *preset_ids, af_setup_verification_row *rows,
                                           int32_t n_streams, hipStream_t stream) {
  const size_t lds = sizeof(double) * (size_t)(T + grid.sort_capacity);
  hipLaunchKernelGGL(sv_shape_kernel, dim3((unsigned)n_streams), dim3(T), lds, stream, grid, freqs, original_db, before_db, after_db,
                     spectrum_stride, after_snr_db, snr_stride, preset_ids, rows);
  return hipGetLastError();
}

hipError_t launch_setup_verification_levels(const SvAudio &audio, af_setup_verification_row *rows, int32_t n_streams, hipStream_t stream) {
  hipLaunchKernelGGL(sv_levels_kernel, dim3((unsigned)n_streams, AF_SETUP_SIGNALS), dim3(T), 0, stream, audio, rows);
  return hipGetLastError();
}

}  // namespace af
