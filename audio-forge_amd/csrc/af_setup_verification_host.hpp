// af_setup_verification_host.hpp -- what the host side and the kernels of the second-passage measurements
// (af_setup_verification.hip) share: the grid's ranges, which depend on the rate and nperseg alone, and the launchers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/audioforge_mi.h"

namespace af {

constexpr int kSvThreads = 256;      // SVM_LANES: the lanes of every sum over bins; four waves, each on one buffer of a signal
constexpr int kSvMaxSorted = 4096;   // doubles one LDS sort holds: the masked bins of nperseg 16384 at 48 kHz are 4070
constexpr int kSvMaxNperseg = 16384;

// the bin ranges of one grid (contiguous: the grid ascends)
struct SvGrid {
  int32_t bins;                          // nperseg / 2 + 1
  int32_t first, count;                  // 80..12000 Hz inclusive, voice_setup.py:1454
  int32_t band_first[4], band_count[4];  // :1637-1643, upper edge exclusive
  int32_t body_count, presence_count, sibilance_count, voice_count;  // target.py:24-26 and :31, within the masked bins
  int32_t sort_capacity;                 // the power of two the sorts pad to
};

// the caller's five signals with the per-stream lengths on the device (or null)
struct SvAudio {
  const float *samples[AF_SETUP_SIGNALS];
  int64_t stride[AF_SETUP_SIGNALS], length[AF_SETUP_SIGNALS];
  const int64_t *lengths[AF_SETUP_SIGNALS];
};

// one workgroup per stream: the two shape errors with their offset scalars, the repeatability delta, the band medians
hipError_t launch_setup_verification_shape(const SvGrid &grid, const double *freqs, const double *original_db, const double *before_db,
                                           const double *after_db, int64_t spectrum_stride, const double *after_snr_db,
                                           int64_t snr_stride, const int32_t *preset_ids, af_setup_verification_row *rows,
                                           int32_t n_streams, hipStream_t stream);
// one workgroup per (stream, signal): sum of squares, peak, flags, rms_db
hipError_t launch_setup_verification_levels(const SvAudio &audio, af_setup_verification_row *rows, int32_t n_streams, hipStream_t stream);

}  // namespace af
