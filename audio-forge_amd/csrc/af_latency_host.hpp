// af_latency_host.hpp -- records, launch geometry and launchers the latency calibration's kernels (af_latency.hip) share with
// their host half (af_api_latency.cpp).  The passes, in launch order on one stream:
//   condition  the mean (NumPy's pairwise order); then, lane per stream, the non-finite flag and the sequential energy prefix
//   score      direct-form normalised correlation: a workgroup scores kLatLagsPerBlock lags against one tile of the reference
//   pick       _pick_peak as reductions; after the whole-probe pick it writes the burst windows the next score launch reads
//   phat       GCC-PHAT: forward real transform, whitened product with the burst's transform, inverse, windowed first-argmax
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "af_latency_math.h"

namespace af {

constexpr int kLatJobs = 1 + LM_MAX_OFFSETS;  // per stream: the whole-probe search, then one window per burst

// condition: the mean by a workgroup per stream, a wave per 8192-sample buffer of NumPy's reduction; then the prefix, kLatCondLanes
// streams per workgroup, a stream per lane of the first wave, the recording and the prefix staged through LDS in tiles of kLatTile
// samples per stream (rows padded by one element: a lane walks its row without bank conflicts)
constexpr int kLatMeanThreads = 256;
constexpr int kLatCondLanes = 64;
constexpr int kLatCondThreads = 256;
constexpr int kLatTile = 128;
constexpr size_t kLatCondLdsBytes = (sizeof(double) + sizeof(float)) * kLatCondLanes * (kLatTile + 1);  // 96.75 KiB

// score: kLatScoreThreads threads of kLatLagsPerThread consecutive lags each; the reference goes through LDS in tiles of
// kLatRefTile terms, the recording in tiles of kLatLagsPerBlock + kLatRefTile terms stored [term % 8][kLatGroupStride] so that
// the lanes of a wave read consecutive doubles (no bank conflict) and 32 consecutive terms are written to 64 distinct banks
constexpr int kLatScoreThreads = 64;
constexpr int kLatLagsPerThread = 8;
constexpr int kLatLagsPerBlock = kLatScoreThreads * kLatLagsPerThread;  // 512
constexpr int kLatRefTile = 256;
constexpr int kLatRecTile = kLatLagsPerBlock + kLatRefTile;  // 768 terms: the last lag's last window term is 504 + 7 + 255
constexpr int kLatGroupStride = 100;                         // >= kLatRecTile / 8, and 4 mod 32
constexpr int kLatPickThreads = 256;

// phat: complex transforms of 2^log_n points, the real transform's half length.  Twiddles come from one host table,
// exp(-2 pi i k / 2^kLatLogTable) for k < 2^(kLatLogTable - 1).
constexpr int kLatLogTable = 18;
constexpr int kLatLdsLogMax = 13;     // one workgroup in LDS up to 8192 complex points: 128 KiB
constexpr int kLatLdsThreads = 512;
constexpr int kLatLogColumns = 8;     // four-step form: 2^log_n = 256 x 2^(log_n - 8); the strided transforms have 256 points,
constexpr int kLatColumnGroup = 8;    // eight neighbours per workgroup so that every global access is a 128-byte segment
constexpr int kLatFourStepThreads = 256;
constexpr size_t kLatWorkspaceBytes = (size_t)256 << 20;  // the four-step form's two buffers per stream: the batch is tiled to fit

struct LatencyJob {
  int32_t lo, count;  // the lags lo .. lo + count - 1
};

struct LatencySearchLags {
  int32_t min_lag, max_lag;
};

struct LatencyArgs {
  const float *rec;        // [n_streams][stride]
  int64_t stride;
  const int32_t *length;   // [n_streams]; 0: the stream took an early exit and no kernel touches it
  lm_record *records;      // [n_streams]
  LatencyJob *jobs;        // [n_streams][kLatJobs]
  const LatencySearchLags *search;  // [n_streams]
  double *prefix;          // [n_streams][prefix_stride]: 0, then the running sum of the centred squares
  int64_t prefix_stride;
  double *full_scores;     // [n_streams][full_stride]
  int64_t full_stride;
  double *burst_scores;    // [n_streams][LM_MAX_OFFSETS][burst_cap]
  double *phat_corr;       // [n_streams][LM_MAX_OFFSETS][burst_cap]
  int32_t burst_cap;
  int32_t n_streams;
  const double *probe, *burst;  // centred, f64
  int32_t probe_len, burst_len;
  double probe_energy, burst_energy;
  int32_t n_offsets, local_radius;
  int32_t offsets[LM_MAX_OFFSETS];
};

// one group of streams that share a transform length
struct LatencyPhatArgs {
  const int32_t *streams;    // [n_group] stream ids
  int32_t n_group;
  int32_t log_n;             // complex points = 2^log_n; real points n = 2^(log_n + 1)
  const double2 *twiddle;    // the host table
  const double2 *burst_spectrum;  // [2^log_n + 1]: rfft(burst, n)
  double2 *work0, *work1;    // four-step form: [n_group][2^log_n] each
  double2 *spectrum_out;     // test hook: [n_group][2^log_n + 1], the forward transform; nothing after it runs
};

hipError_t launch_latency_condition(const LatencyArgs &a, hipStream_t stream);
// kind 0: job 0 against the probe; kind 1: jobs 1.. against the burst.  `lags`: the longest job's count.
hipError_t launch_latency_score(const LatencyArgs &a, int kind, int32_t lags, hipStream_t stream);
hipError_t launch_latency_pick(const LatencyArgs &a, int kind, hipStream_t stream);
hipError_t launch_latency_phat(const LatencyArgs &a, const LatencyPhatArgs &p, hipStream_t stream);

}  // namespace af
