// af_latency.hip -- the kernels of the latency calibration (python/mic_eq/analysis/latency_calibration.py), f64 throughout,
// unfused (-ffp-contract=off).  Geometry and records: af_latency_host.hpp; sum orders and per-element rules: af_latency_math.h.
//   lat_mean_kernel       np.mean in NumPy's pairwise order, a workgroup per stream: the leaves by lm_sum (the host's own code), the
//                         levels above them in LDS.
//   lat_condition_kernel  64 streams per workgroup, a stream per lane of its first wave: the energy prefix is np.cumsum's running
//                         sum; four waves stage the recording and the prefix through LDS in 128-sample tiles (512-byte runs).
//   lat_score_kernel      _normalized_correlation_scores (:137-168) as a direct sum: 64 threads x 8 consecutive lags, a sliding
//                         register window over the recording tile, the reference tile broadcast from LDS; 16 LDS reads per 64
//                         multiply-adds.
//   lat_pick_kernel       _pick_peak (:201-229) as reductions, then (after the whole-probe pick) the burst windows of :360-362.
//   lat_phat_*            _phat_lag_hint (:171-198): the real transform of n points as a complex one of n / 2; one workgroup in LDS
//                         up to 8192 complex points, the four-step form (256-point strided transforms, twiddle, transposed row
//                         transforms) through global memory above that.  Radix 2, twiddles from the host's table.
#include <hip/hip_runtime.h>

#define SVM_FN __host__ __device__ static inline
#define LM_FN __host__ __device__ static inline
#include "af_latency_host.hpp"

namespace af {
namespace {

__device__ inline bool lat_active(const LatencyArgs &a, int s) { return a.length[s] > 0 && !a.records[s].non_finite; }

// ---- condition -------------------------------------------------------------------------------------------------------------
// np.mean of one stream per workgroup, NumPy's order: a wave takes a buffer of 8192 samples, its lane l the node that the bits of
// l, most significant first, lead to from the buffer's root (the layout of sv_levels_kernel, af_setup_verification.hip), sums it
// with lm_sum, and the six levels above are added in LDS, left + right; thread 0 adds the buffers in order.
__global__ __launch_bounds__(kLatMeanThreads) void lat_mean_kernel(LatencyArgs a) {
  __shared__ double red[kLatMeanThreads];
  __shared__ int here[kLatMeanThreads];
  __shared__ double buffers[AF_LATENCY_MAX_TRANSFORM / SVM_PAIRWISE_BUFFER];
  const int t = (int)threadIdx.x, lane = t % 64, wave = t / 64, s = (int)blockIdx.x;
  const int64_t n = a.length[s];
  if (n <= 0) return;
  const float *x = a.rec + (int64_t)s * a.stride;
  constexpr int kWaves = kLatMeanThreads / 64;
  for (int64_t base = 0; base < n; base += (int64_t)kWaves * SVM_PAIRWISE_BUFFER) {
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
    red[t] = present ? lm_sum(x + start + lo, len) : 0.0;
    here[t] = present;
    __syncthreads();
    for (int h = 1; h < 64; h *= 2) {
      if (lane % (2 * h) == 0 && here[t + h]) red[t] = red[t] + red[t + h];
      __syncthreads();
    }
    if (lane == 0 && start < n) buffers[start / SVM_PAIRWISE_BUFFER] = red[t];
    __syncthreads();
  }
  if (t == 0) {
    double total = 0.0;
    for (int64_t b = 0; b * SVM_PAIRWISE_BUFFER < n; ++b) total += buffers[b];
    a.records[s].mean = total / (double)n;  // np.mean: add.reduce / count
  }
}

// the non-finite flag and np.cumsum(rec * rec), 64 streams per workgroup.  The running sum is serial per stream: lane l of the
// first wave owns stream l.  All four waves move the tiles (kLatTile samples of each stream, whole 512-byte runs) between global
// memory and LDS, so that a tile's memory latency is paid once per 128 dependent adds.
__global__ __launch_bounds__(kLatCondThreads) void lat_condition_kernel(LatencyArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lat_cond_lds[];
  double(*tout)[kLatTile + 1] = reinterpret_cast<double(*)[kLatTile + 1]>(lat_cond_lds);
  float(*tin)[kLatTile + 1] = reinterpret_cast<float(*)[kLatTile + 1]>(lat_cond_lds + sizeof(double) * kLatCondLanes * (kLatTile + 1));
  __shared__ int32_t lens[kLatCondLanes];
  const int t = (int)threadIdx.x, s0 = (int)blockIdx.x * kLatCondLanes, s = s0 + t;
  const bool owner = t < kLatCondLanes;
  const int32_t n = owner && s < a.n_streams ? a.length[s] : 0;
  if (owner) lens[t] = n;
  __syncthreads();
  int32_t longest = 0;
  for (int l = 0; l < kLatCondLanes; ++l) longest = lens[l] > longest ? lens[l] : longest;
  const double mean = n > 0 ? a.records[s].mean : 0.0;
  double acc = 0.0;
  int bad = 0;
  if (n > 0) a.prefix[(int64_t)s * a.prefix_stride] = 0.0;
  constexpr int kMoves = kLatCondLanes * kLatTile / kLatCondThreads;
  for (int32_t t0 = 0; t0 < longest; t0 += kLatTile) {
#pragma unroll
    for (int it = 0; it < kMoves; ++it) {
      const int idx = it * kLatCondThreads + t, row = idx / kLatTile, col = idx % kLatTile;
      tin[row][col] = t0 + col < lens[row] ? a.rec[(int64_t)(s0 + row) * a.stride + t0 + col] : 0.0f;
    }
    __syncthreads();
    if (owner)
      for (int k0 = 0; k0 < kLatTile; k0 += 8) {  // eight LDS reads ahead of the dependent adds
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = tin[t][k0 + j];
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (t0 + k0 + j < n) {
            const double d = (double)v[j] - mean;
            bad |= !isfinite(v[j]);
            acc += d * d;
            tout[t][k0 + j] = acc;
          }
      }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < kMoves; ++it) {
      const int idx = it * kLatCondThreads + t, row = idx / kLatTile, col = idx % kLatTile;
      if (t0 + col < lens[row]) a.prefix[(int64_t)(s0 + row) * a.prefix_stride + t0 + col + 1] = tout[row][col];
    }
    __syncthreads();
  }
  if (owner && s < a.n_streams) a.records[s].non_finite = bad;
}

// ---- score -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLatScoreThreads) void lat_score_kernel(LatencyArgs a, int kind) {
  __shared__ double rec_s[8 * kLatGroupStride];
  __shared__ double ref_s[kLatRefTile];
  const int t = (int)threadIdx.x, s = (int)blockIdx.z, job = kind ? 1 + (int)blockIdx.y : 0;
  const int32_t base = (int32_t)blockIdx.x * kLatLagsPerBlock;
  if (!lat_active(a, s)) return;
  const LatencyJob J = a.jobs[s * kLatJobs + job];
  if (base >= J.count) return;
  const double *ref = kind ? a.burst : a.probe;
  const int32_t ref_len = kind ? a.burst_len : a.probe_len, len = a.length[s];
  const double ref_energy = kind ? a.burst_energy : a.probe_energy, mean = a.records[s].mean;
  const float *x = a.rec + (int64_t)s * a.stride;
  double acc[kLatLagsPerThread];
  for (int j = 0; j < kLatLagsPerThread; ++j) acc[j] = 0.0;
  for (int32_t k0 = 0; k0 < ref_len; k0 += kLatRefTile) {
    const int32_t kt = ref_len - k0 < kLatRefTile ? ref_len - k0 : kLatRefTile, groups = (kt + 7) / 8;
    for (int e = t; e < kLatRefTile; e += kLatScoreThreads) ref_s[e] = e < kt ? ref[k0 + e] : 0.0;
    for (int e = t; e < kLatRecTile; e += kLatScoreThreads) {
      const int64_t at = (int64_t)J.lo + base + k0 + e;  // J.lo >= 0
      rec_s[(e % 8) * kLatGroupStride + e / 8] = at < len ? (double)x[at] - mean : 0.0;
    }
    __syncthreads();
    double w[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = rec_s[i * kLatGroupStride + t];
    for (int c = 0; c < groups; ++c) {
#pragma unroll
      for (int i = 0; i < 8; ++i) w[8 + i] = rec_s[i * kLatGroupStride + t + c + 1];
#pragma unroll
      for (int kp = 0; kp < 8; ++kp) {
        const double r = ref_s[c * 8 + kp];
#pragma unroll
        for (int j = 0; j < kLatLagsPerThread; ++j) acc[j] = acc[j] + w[j + kp] * r;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) w[i] = w[8 + i];
    }
    __syncthreads();
  }
  double *out = kind ? a.burst_scores + ((int64_t)s * LM_MAX_OFFSETS + (job - 1)) * a.burst_cap : a.full_scores + (int64_t)s * a.full_stride;
  const double *prefix = a.prefix + (int64_t)s * a.prefix_stride;
  for (int j = 0; j < kLatLagsPerThread; ++j) {
    const int32_t li = base + t * kLatLagsPerThread + j;
    if (li < J.count) {
      const int64_t lag = (int64_t)J.lo + li;  // lag + ref_len <= len: the job's lags are inside the capture
      out[li] = lm_score(acc[j], prefix[lag + ref_len] - prefix[lag], ref_energy);
    }
  }
}

// ---- pick ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLatPickThreads) void lat_pick_kernel(LatencyArgs a, int kind) {
  __shared__ double red[kLatPickThreads];
  __shared__ int32_t redi[kLatPickThreads];
  const int t = (int)threadIdx.x, s = (int)blockIdx.y, job = kind ? 1 + (int)blockIdx.x : 0;
  if (!lat_active(a, s)) return;
  const LatencyJob J = a.jobs[s * kLatJobs + job];
  lm_record *rec = a.records + s;
  if (J.count <= 0) return;  // an empty window: the record's count says so
  const double *scores = kind ? a.burst_scores + ((int64_t)s * LM_MAX_OFFSETS + (job - 1)) * a.burst_cap : a.full_scores + (int64_t)s * a.full_stride;
  const double bias = kind ? LM_BURST_BIAS : LM_FULL_BIAS;
  double m = 0.0;  // scores are >= 0
  for (int32_t i = t; i < J.count; i += kLatPickThreads) m = scores[i] > m ? scores[i] : m;
  red[t] = m;
  __syncthreads();
  for (int h = kLatPickThreads / 2; h >= 1; h /= 2) {
    if (t < h) red[t] = red[t + h] > red[t] ? red[t + h] : red[t];
    __syncthreads();
  }
  const double threshold = red[0] * bias;
  __syncthreads();
  int32_t first = J.count;
  for (int32_t i = t; i < J.count; i += kLatPickThreads)
    if (scores[i] >= threshold) { first = i; break; }
  redi[t] = first;
  __syncthreads();
  for (int h = kLatPickThreads / 2; h >= 1; h /= 2) {
    if (t < h) redi[t] = redi[t + h] < redi[t] ? redi[t + h] : redi[t];
    __syncthreads();
  }
  const int32_t index = redi[0] < J.count ? redi[0] : 0;
  const int32_t radius = lm_exclusion_radius(J.count);
  m = 0.0;  // off-peak scores are >= 0 and an empty off-peak set gives 0.0, :226
  for (int32_t i = t; i < J.count; i += kLatPickThreads)
    if (i < index - radius || i > index + radius) m = scores[i] > m ? scores[i] : m;
  red[t] = m;
  __syncthreads();
  for (int h = kLatPickThreads / 2; h >= 1; h /= 2) {
    if (t < h) red[t] = red[t + h] > red[t] ? red[t + h] : red[t];
    __syncthreads();
  }
  if (t != 0) return;
  const double offset = index > 0 && index < J.count - 1 ? lm_parabolic_offset(scores[index - 1], scores[index], scores[index + 1]) : 0.0;
  const lm_pick pick = lm_pick_from((double)(J.lo + index), offset, scores[index], red[0]);
  if (kind) {
    rec->burst[job - 1] = pick;
    return;
  }
  rec->full = pick;
  rec->full_count = J.count;
  const int32_t len = a.length[s];
  for (int k = 0; k < LM_MAX_OFFSETS; ++k) {
    int32_t lag_min = 0, lag_max = -1, lo = 0, count = 0;
    if (k < a.n_offsets) {
      lm_burst_window(pick.peak_lag, a.offsets[k], a.local_radius, a.search[s].min_lag, a.search[s].max_lag, &lag_min, &lag_max);
      lo = lag_min > 0 ? lag_min : 0;
      const int32_t hi = lag_max < len - a.burst_len ? lag_max : len - a.burst_len;
      count = hi >= lo ? hi - lo + 1 : 0;
      if (count > a.burst_cap) count = a.burst_cap;  // cannot happen: the window has at most 2 radius + 2 lags
    }
    a.jobs[s * kLatJobs + 1 + k] = LatencyJob{lo, count};
    rec->lag_min[k] = lag_min;
    rec->lag_max[k] = lag_max;
    rec->burst_lo[k] = lo;
    rec->burst_count[k] = count;
    rec->phat_count[k] = 0;
  }
}

// ---- phat ------------------------------------------------------------------------------------------------------------------
__device__ inline double2 cmul(double2 a, double2 b) { return double2{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ inline double2 cadd(double2 a, double2 b) { return double2{a.x + b.x, a.y + b.y}; }
__device__ inline double2 csub(double2 a, double2 b) { return double2{a.x - b.x, a.y - b.y}; }
__device__ inline double2 cconj(double2 a) { return double2{a.x, -a.y}; }

// exp(-2 pi i e / 2^kLatLogTable) for e in [0, 2^kLatLogTable), conjugated for the inverse
template <bool INV>
__device__ inline double2 lat_twiddle(const double2 *table, uint32_t e) {
  constexpr uint32_t half = 1u << (kLatLogTable - 1);
  double2 w = table[e & (half - 1)];
  if (e & half) w = double2{-w.x, -w.y};
  if (INV) w.y = -w.y;
  return w;
}

// in place, radix 2, decimation in time: `s` holds 2^log_n points in bit-reversed order (`count` transforms of that size, one
// after the other) and leaves them in natural order
template <bool INV>
__device__ void lat_fft_lds(double2 *s, int log_n, int count, const double2 *table, int t, int threads) {
  const int half_points = 1 << (log_n - 1), butterflies = count << (log_n - 1);
  for (int st = 1; st <= log_n; ++st) {
    const int half = 1 << (st - 1);
    for (int b = t; b < butterflies; b += threads) {
      const int which = b >> (log_n - 1), bb = b & (half_points - 1), j = bb & (half - 1);
      const int i0 = (which << log_n) + ((bb >> (st - 1)) << st) + j, i1 = i0 + half;
      const double2 w = lat_twiddle<INV>(table, (uint32_t)j << (kLatLogTable - st));
      const double2 u = s[i0], v = cmul(s[i1], w);
      s[i0] = cadd(u, v);
      s[i1] = csub(u, v);
    }
    __syncthreads();
  }
}

__device__ inline uint32_t lat_bitrev(uint32_t i, int bits) { return __brev(i) >> (32 - bits); }

// the packed input of the real transform: z[m] = rec[2 m] + i rec[2 m + 1], centred, zero past the recording
__device__ inline double2 lat_packed(const float *x, int32_t len, double mean, int64_t m) {
  double2 z;
  z.x = 2 * m < len ? (double)x[2 * m] - mean : 0.0;
  z.y = 2 * m + 1 < len ? (double)x[2 * m + 1] - mean : 0.0;
  return z;
}

// From Z = FFT(z) at k and N - k (a thread owns the pair; k <= N / 2): X = rfft(rec) at both, the whitened cross spectrum with
// the burst (:187-188), and the packed input of the inverse, scaled by 1 / (2 N) (the packing's half and the inverse's 1 / N) so that the inverse transform needs no scale.
// zk = Z[k], zn = Z[(N - k) % N]; on return zk = Z'[k], zn = Z'[N - k] (for k = 0 only zk is meaningful).
__device__ inline void lat_phat_pair(double2 &zk, double2 &zn, uint32_t k, int log_n, const double2 *table, const double2 *burst_spectrum,
                                     double2 *spectrum_out) {
  const uint32_t N = 1u << log_n;
  const double2 w = lat_twiddle<false>(table, k << (kLatLogTable - 1 - log_n));  // exp(-2 pi i k / 2N)
  // X[k] = E + w O, X[N - k] = conj(E) - conj(w) conj(O) with E = (Z[k] + conj(Z[N-k])) / 2, O = -i (Z[k] - conj(Z[N-k])) / 2
  const double2 zc = cconj(zn);
  const double2 e = double2{(zk.x + zc.x) * 0.5, (zk.y + zc.y) * 0.5};
  const double2 d = csub(zk, zc);
  const double2 o = double2{d.y * 0.5, -d.x * 0.5};
  const double2 wo = cmul(w, o);
  double2 xk = cadd(e, wo), xn = cconj(csub(e, wo));
  if (spectrum_out) {
    spectrum_out[k] = xk;
    spectrum_out[N - k] = xn;
    return;
  }
  double2 y[2] = {xk, xn};
  const uint32_t at[2] = {k, N - k};
  for (int q = 0; q < 2; ++q) {
    const double2 c = cmul(y[q], cconj(burst_spectrum[at[q]]));
    const double mag = hypot(c.x, c.y);
    const double scale = 1.0 / (mag > 1e-12 ? mag : 1e-12);  // NumPy divides a complex by a real through its reciprocal
    y[q] = double2{c.x * scale, c.y * scale};
  }
  if (k == 0) { y[0].y = 0.0; y[1].y = 0.0; }  // irfft reads the real parts of the two ends only
  // Z'[k] = ((Y[k] + conj(Y[N-k])) + i (Y[k] - conj(Y[N-k])) conj(w)) / 2, Z'[N-k] likewise with the roles swapped
  const double scale = 0.5 / (double)N;
  const double2 yc = cconj(y[1]);
  const double2 sum = cadd(y[0], yc), dif = cmul(csub(y[0], yc), cconj(w));
  zk = double2{(sum.x - dif.y) * scale, (sum.y + dif.x) * scale};
  // at N - k: Y[N-k] + conj(Y[k]) = conj(sum); (Y[N-k] - conj(Y[k])) exp(+2 pi i (N-k) / 2N) = conj(dif) (the sign and the
  // conjugate twiddle cancel: exp(i pi (N-k)/N) = -conj(exp(i pi k/N)))
  zn = double2{(sum.x + dif.y) * scale, (-sum.y + dif.x) * scale};
}

// the windowed first-argmax of |corr| per burst (:190-198) by the whole workgroup; corr holds n real points
__device__ void lat_phat_windows(const LatencyArgs &a, int s, const double *corr, int64_t n, double *red, int32_t *redi, int t, int threads) {
  lm_record *rec = a.records + s;
  for (int k = 0; k < a.n_offsets; ++k) {
    const int64_t lo = rec->lag_min[k] > -(n / 2 - 1) ? rec->lag_min[k] : -(n / 2 - 1);
    const int64_t hi = rec->lag_max[k] < n / 2 ? rec->lag_max[k] : n / 2;
    int64_t count = hi >= lo ? hi - lo + 1 : 0;
    if (count > a.burst_cap) count = a.burst_cap;
    double *out = a.phat_corr + ((int64_t)s * LM_MAX_OFFSETS + k) * a.burst_cap;
    double best = -1.0;
    int32_t best_at = 0x7fffffff;
    for (int64_t i = t; i < count; i += threads) {
      const int64_t lag = lo + i, at = lag >= 0 ? lag : n + lag;
      const double v = corr[at];
      out[i] = v;
      if (fabs(v) > best || (fabs(v) == best && (int32_t)at < best_at)) { best = fabs(v); best_at = (int32_t)at; }
    }
    red[t] = best;
    redi[t] = best_at;
    __syncthreads();
    for (int h = threads / 2; h >= 1; h /= 2) {
      if (t < h && (red[t + h] > red[t] || (red[t + h] == red[t] && redi[t + h] < redi[t]))) { red[t] = red[t + h]; redi[t] = redi[t + h]; }
      __syncthreads();
    }
    if (t == 0) {
      rec->phat_lo[k] = (int32_t)lo;
      rec->phat_count[k] = (int32_t)count;
      rec->phat_hint[k] = count > 0 ? (redi[0] > n / 2 ? (int32_t)(redi[0] - n) : redi[0]) : 0;
    }
    __syncthreads();
  }
}

// one workgroup per stream, everything in LDS
__global__ __launch_bounds__(kLatLdsThreads) void lat_phat_lds_kernel(LatencyArgs a, LatencyPhatArgs p) {
  extern __shared__ __attribute__((aligned(16))) double2 lat_lds[];  // [2^log_n]
  __shared__ double red[kLatLdsThreads];
  __shared__ int32_t redi[kLatLdsThreads];
  const int t = (int)threadIdx.x, s = p.streams[blockIdx.x];
  if (!lat_active(a, s)) return;
  const uint32_t N = 1u << p.log_n;
  const float *x = a.rec + (int64_t)s * a.stride;
  const int32_t len = a.length[s];
  const double mean = a.records[s].mean;
  for (uint32_t m = t; m < N; m += kLatLdsThreads) lat_lds[lat_bitrev(m, p.log_n)] = lat_packed(x, len, mean, m);
  __syncthreads();
  lat_fft_lds<false>(lat_lds, p.log_n, 1, p.twiddle, t, kLatLdsThreads);
  double2 *spectrum_out = p.spectrum_out ? p.spectrum_out + (int64_t)blockIdx.x * (N + 1) : nullptr;
  for (uint32_t k = t; k <= N / 2; k += kLatLdsThreads) {
    double2 zk = lat_lds[k], zn = lat_lds[(N - k) & (N - 1)];
    lat_phat_pair(zk, zn, k, p.log_n, p.twiddle, p.burst_spectrum, spectrum_out);
    lat_lds[k] = zk;
    if (k != 0 && k != N / 2) lat_lds[N - k] = zn;
  }
  __syncthreads();
  if (spectrum_out) return;
  for (uint32_t i = t; i < N; i += kLatLdsThreads) {  // into bit-reversed order for the inverse
    const uint32_t j = lat_bitrev(i, p.log_n);
    if (i < j) { const double2 u = lat_lds[i]; lat_lds[i] = lat_lds[j]; lat_lds[j] = u; }
  }
  __syncthreads();
  lat_fft_lds<true>(lat_lds, p.log_n, 1, p.twiddle, t, kLatLdsThreads);
  lat_phat_windows(a, s, reinterpret_cast<const double *>(lat_lds), (int64_t)2 * N, red, redi, t, kLatLdsThreads);
}

// four-step, first half: the 256-point transforms down the columns n2 = c0 .. c0 + 7 of the [256][N2] view, times
// exp(-+2 pi i n2 k1 / N); REAL: the input is the packed recording, else `in`.  Output [k1][n2].
template <bool INV, bool REAL>
__global__ __launch_bounds__(kLatFourStepThreads) void lat_fft_columns_kernel(LatencyArgs a, LatencyPhatArgs p) {
  __shared__ double2 s_[kLatColumnGroup << kLatLogColumns];  // [8][256]: 32 KiB
  const int t = (int)threadIdx.x, g = (int)blockIdx.y, s = p.streams[g];
  if (!lat_active(a, s)) return;
  const uint32_t N = 1u << p.log_n, N2 = N >> kLatLogColumns, c0 = blockIdx.x * kLatColumnGroup;
  const float *x = a.rec + (int64_t)s * a.stride;
  const int32_t len = a.length[s];
  const double mean = a.records[s].mean;
  const double2 *in = p.work1 + (int64_t)g * N;
  double2 *out = p.work0 + (int64_t)g * N;
  for (uint32_t idx = t; idx < (kLatColumnGroup << kLatLogColumns); idx += kLatFourStepThreads) {
    const uint32_t j = idx % kLatColumnGroup, n1 = idx / kLatColumnGroup, m = n1 * N2 + c0 + j;
    s_[(j << kLatLogColumns) + lat_bitrev(n1, kLatLogColumns)] = REAL ? lat_packed(x, len, mean, m) : in[m];
  }
  __syncthreads();
  lat_fft_lds<INV>(s_, kLatLogColumns, kLatColumnGroup, p.twiddle, t, kLatFourStepThreads);
  for (uint32_t idx = t; idx < (kLatColumnGroup << kLatLogColumns); idx += kLatFourStepThreads) {
    const uint32_t j = idx % kLatColumnGroup, k1 = idx / kLatColumnGroup, n2 = c0 + j;
    const double2 w = lat_twiddle<INV>(p.twiddle, ((n2 * k1) & (N - 1)) << (kLatLogTable - p.log_n));
    out[k1 * N2 + n2] = cmul(s_[(j << kLatLogColumns) + k1], w);
  }
}

// four-step, second half: the N2-point transforms along the rows k1 = r0 .. r0 + 7, stored transposed: X[k1 + 256 k2]
template <bool INV>
__global__ __launch_bounds__(kLatFourStepThreads) void lat_fft_rows_kernel(LatencyArgs a, LatencyPhatArgs p) {
  extern __shared__ __attribute__((aligned(16))) double2 lat_lds[];  // [8][N2]
  const int t = (int)threadIdx.x, g = (int)blockIdx.y, s = p.streams[g];
  if (!lat_active(a, s)) return;
  const uint32_t N = 1u << p.log_n, N2 = N >> kLatLogColumns, r0 = blockIdx.x * kLatColumnGroup;
  const int log_n2 = p.log_n - kLatLogColumns;
  const double2 *in = p.work0 + (int64_t)g * N;
  double2 *out = p.work1 + (int64_t)g * N;
  for (uint32_t idx = t; idx < kLatColumnGroup * N2; idx += kLatFourStepThreads) {
    const uint32_t j = idx / N2, n2 = idx % N2;
    lat_lds[j * N2 + lat_bitrev(n2, log_n2)] = in[(r0 + j) * N2 + n2];
  }
  __syncthreads();
  lat_fft_lds<INV>(lat_lds, log_n2, kLatColumnGroup, p.twiddle, t, kLatFourStepThreads);
  for (uint32_t idx = t; idx < kLatColumnGroup * N2; idx += kLatFourStepThreads) {
    const uint32_t j = idx % kLatColumnGroup, k2 = idx / kLatColumnGroup;
    out[(r0 + j) + (k2 << kLatLogColumns)] = lat_lds[j * N2 + k2];
  }
}

// four-step, between the transforms: work1 holds Z, and receives Z'
__global__ __launch_bounds__(kLatFourStepThreads) void lat_phat_mid_kernel(LatencyArgs a, LatencyPhatArgs p) {
  const int g = (int)blockIdx.y, s = p.streams[g];
  if (!lat_active(a, s)) return;
  const uint32_t N = 1u << p.log_n, k = blockIdx.x * kLatFourStepThreads + threadIdx.x;
  if (k > N / 2) return;
  double2 *z = p.work1 + (int64_t)g * N;
  double2 zk = z[k], zn = z[(N - k) & (N - 1)];
  lat_phat_pair(zk, zn, k, p.log_n, p.twiddle, p.burst_spectrum, p.spectrum_out ? p.spectrum_out + (int64_t)g * (N + 1) : nullptr);
  if (p.spectrum_out) return;
  z[k] = zk;
  if (k != 0 && k != N / 2) z[N - k] = zn;
}

__global__ __launch_bounds__(kLatPickThreads) void lat_phat_window_kernel(LatencyArgs a, LatencyPhatArgs p) {
  __shared__ double red[kLatPickThreads];
  __shared__ int32_t redi[kLatPickThreads];
  const int g = (int)blockIdx.x, s = p.streams[g];
  if (!lat_active(a, s)) return;
  const int64_t N = (int64_t)1 << p.log_n;
  lat_phat_windows(a, s, reinterpret_cast<const double *>(p.work1 + g * N), 2 * N, red, redi, (int)threadIdx.x, kLatPickThreads);
}

template <class K>
hipError_t lat_allow_lds(K kernel, size_t bytes) {
  return bytes > 64 * 1024 ? hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes)
                           : hipSuccess;
}

}  // namespace

hipError_t launch_latency_condition(const LatencyArgs &a, hipStream_t stream) {
  lat_mean_kernel<<<dim3(a.n_streams), dim3(kLatMeanThreads), 0, stream>>>(a);
  if (hipError_t err = lat_allow_lds(lat_condition_kernel, kLatCondLdsBytes); err != hipSuccess) return err;
  lat_condition_kernel<<<dim3((a.n_streams + kLatCondLanes - 1) / kLatCondLanes), dim3(kLatCondThreads), kLatCondLdsBytes, stream>>>(a);
  return hipGetLastError();
}

hipError_t launch_latency_score(const LatencyArgs &a, int kind, int32_t lags, hipStream_t stream) {
  if (lags <= 0) return hipSuccess;
  const dim3 grid((lags + kLatLagsPerBlock - 1) / kLatLagsPerBlock, kind ? a.n_offsets : 1, a.n_streams);
  lat_score_kernel<<<grid, dim3(kLatScoreThreads), 0, stream>>>(a, kind);
  return hipGetLastError();
}

hipError_t launch_latency_pick(const LatencyArgs &a, int kind, hipStream_t stream) {
  lat_pick_kernel<<<dim3(kind ? a.n_offsets : 1, a.n_streams), dim3(kLatPickThreads), 0, stream>>>(a, kind);
  return hipGetLastError();
}

hipError_t launch_latency_phat(const LatencyArgs &a, const LatencyPhatArgs &p, hipStream_t stream) {
  const size_t points = (size_t)1 << p.log_n;
  if (p.log_n <= kLatLdsLogMax) {
    const size_t lds = points * sizeof(double2);
    if (hipError_t err = lat_allow_lds(lat_phat_lds_kernel, lds); err != hipSuccess) return err;
    lat_phat_lds_kernel<<<dim3(p.n_group), dim3(kLatLdsThreads), lds, stream>>>(a, p);
    return hipGetLastError();
  }
  const size_t n2 = points >> kLatLogColumns, lds = kLatColumnGroup * n2 * sizeof(double2);
  const dim3 columns((unsigned)(n2 / kLatColumnGroup), p.n_group), rows((1u << kLatLogColumns) / kLatColumnGroup, p.n_group);
  const dim3 mid((unsigned)((points / 2 + kLatFourStepThreads) / kLatFourStepThreads), p.n_group), threads(kLatFourStepThreads);
  if (hipError_t err = lat_allow_lds(lat_fft_rows_kernel<false>, lds); err != hipSuccess) return err;
  if (hipError_t err = lat_allow_lds(lat_fft_rows_kernel<true>, lds); err != hipSuccess) return err;
  lat_fft_columns_kernel<false, true><<<columns, threads, 0, stream>>>(a, p);
  lat_fft_rows_kernel<false><<<rows, threads, lds, stream>>>(a, p);
  lat_phat_mid_kernel<<<mid, threads, 0, stream>>>(a, p);
  if (!p.spectrum_out) {
    lat_fft_columns_kernel<true, false><<<columns, threads, 0, stream>>>(a, p);
    lat_fft_rows_kernel<true><<<rows, threads, lds, stream>>>(a, p);
    lat_phat_window_kernel<<<dim3(p.n_group), dim3(kLatPickThreads), 0, stream>>>(a, p);
  }
  return hipGetLastError();
}

}  // namespace af
