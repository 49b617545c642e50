// af_resampler.hip -- batched asynchronous sinc resampler for gfx950 (the product resampler of
// rust-core/src/audio/processor/resampling.rs:140-261 over rubato's SincFixedIn, see af_resampler_host.hpp).
//
// Work decomposition.  Output positions are the same for every stream, so a workgroup takes 64 streams
// (lane = stream) x one segment of consecutive outputs:
//   1. the input span the segment reads (segment * 1/ratio + sinc_len + 3 frames) moves HBM -> LDS once,
//      transposed to [time][stream] (each stream row is read as coalesced 512 B pieces; 65-double rows keep
//      the transposing writes at the natural 2-way bank split of 8-byte accesses);
//   2. each wave takes a run of outputs, two at a time; per output the four sinc rows are WAVE-UNIFORM (scalar
//      loads, SGPR operands), the signal is one conflict-free ds_read_b64 per tap shared by the eight rows of
//      the pair, and the arithmetic is 4 x sinc_len f64 FMAs per output per lane -- the kernel is bound by the
//      f64 VALU rate (512 FMA per output frame at sinc_len 128), not by HBM: 16 B of audio per 1 kFLOP.
//      (One output per pass read LDS once per 4 FMAs, which saturates the LDS pipe exactly when the VALU
//      saturates; pairing halves that.)
//   3. results go back through LDS so that the store is again coalesced along time.
// Every sinc row is stored with eight zero taps either side, so the window offsets of the four points (0..2
// frames) and of the pair's second output (its window starts 0..6 frames later) need no branches: a zero tap
// leaves the accumulator unchanged, and each accumulator is one fused multiply-add chain over the taps in
// increasing order -- the oracle's order, so the two agree bit for bit.
#include <hip/hip_runtime.h>

#include "af_resampler_body.h"

namespace af {

struct ResampleArgs {
  const double *in;
  double *out;
  const ResamplePos *pos;   // [n_out]
  const double *table;      // [256][sinc_len + 4]
  int64_t n_in, n_out, in_stride, out_stride;
  int32_t n_streams, sinc_len, max_rows;
};

// The one-shot job's audio: f64 clips in global memory, frames outside [0, n_in) are zeros (the reference's zero history, its
// zero-padded partial chunk and its silent flush chunks).  The compute bodies are in af_resampler_body.h.
struct ResampleIoF64 {
  const double *in;
  double *out;
  int64_t n_in, in_stride, out_stride;
  struct InRow {
    const double *src;
    int64_t n_in;
    __device__ __forceinline__ double at(int64_t g) const { return (g >= 0 && g < n_in) ? src[g] : 0.0; }
  };
  struct OutRow {
    double *dst;
    __device__ __forceinline__ void put(int64_t o, double v) const { dst[o] = v; }
  };
  __device__ __forceinline__ InRow in_row(int s) const { return InRow{in + (int64_t)s * in_stride, n_in}; }
  __device__ __forceinline__ OutRow out_row(int s) const { return OutRow{out + (int64_t)s * out_stride}; }
};

template <int kWaves, int kOutPerWave>
__global__ __launch_bounds__(kWaves *kResLanes) void resample_kernel(ResampleArgs a) {
  extern __shared__ double lds[];  // [max(rows, segment outputs)][65]
  const ResampleCore core{a.pos, a.table, a.n_out, a.n_streams, a.sinc_len, a.max_rows};
  const ResampleIoF64 io{a.in, a.out, a.n_in, a.in_stride, a.out_stride};
  resample_valu_body<kWaves, kOutPerWave>(core, io, lds);
}

template <int kGroups>
__global__ __launch_bounds__(kGroups * 4 * kResLanes) void resample_mfma_kernel(ResampleArgs a) {
  extern __shared__ double lds[];  // [kGroups][kMfRows][16 streams]; later [128 outputs][kStreams + 1]
  const ResampleCore core{a.pos, a.table, a.n_out, a.n_streams, a.sinc_len, a.max_rows};
  const ResampleIoF64 io{a.in, a.out, a.n_in, a.in_stride, a.out_stride};
  resample_mfma_body<kGroups>(core, io, lds);
}

template <int kGroups>
static hipError_t launch_resample_mfma_variant(const ResampleArgs &a, hipStream_t stream) {
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(resample_mfma_kernel<kGroups>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (err != hipSuccess) return err;
    attr_set = true;
  }
  const size_t dyn = sizeof(double) * kGroups * kMfRows * 16;
  const dim3 grid((unsigned)((a.n_out + kMfSeg - 1) / kMfSeg), (unsigned)((a.n_streams + 16 * kGroups - 1) / (16 * kGroups)));
  hipLaunchKernelGGL(resample_mfma_kernel<kGroups>, grid, dim3(kGroups * 4 * kResLanes), dyn, stream, a);
  return hipGetLastError();
}
// the matrix-core tile needs: 128 outputs' span + the tap round-up inside 288 rows, and a tile's four windows
// starting within 8 frames of each other (row padding 16)
bool resample_mfma_ok(double ratio, int sinc_len) {
  return std::ceil(128.0 / ratio) + sinc_len + 14 <= kMfRows && 3.0 / ratio + 3.0 <= 8.0;  // (128 x 33 staging fits 2 x 288 x 16)
}

template <int kWaves, int kOutPerWave>
static hipError_t launch_resample_variant(const ResampleArgs &a, hipStream_t stream) {
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(resample_kernel<kWaves, kOutPerWave>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (err != hipSuccess) return err;
    attr_set = true;
  }
  constexpr int kSeg = kWaves * kOutPerWave;
  const size_t dyn = sizeof(double) * kResRowStride * (size_t)kResMaxRows;
  const dim3 grid((unsigned)((a.n_out + kSeg - 1) / kSeg), (unsigned)((a.n_streams + kResLanes - 1) / kResLanes));
  hipLaunchKernelGGL((resample_kernel<kWaves, kOutPerWave>), grid, dim3(kWaves * kResLanes), dyn, stream, a);
  return hipGetLastError();
}

// Largest segment whose input span fits the LDS tile: span = ceil(segment / ratio) + sinc_len + 3 frames.
int resample_segment_outputs(double ratio, int sinc_len) {
  if (1.0 / ratio > 5.0) return 0;  // a pair's second window may start at most 6 frames after the first (row padding)
  const int candidates[] = {128, 64, 32, 16, 8};
  for (int seg : candidates) {
    const double span = std::ceil((double)seg / ratio) + sinc_len + 4;
    if (span <= kResMaxRows && seg <= kResMaxRows) return seg;
  }
  return 0;
}

ResampleForm resample_pick_form(double ratio, int sinc_len, int variant) {
  if (variant != 1 && resample_mfma_ok(ratio, sinc_len)) return ResampleForm{1, kMfSeg, variant == 2 ? 32 : 64};
  return ResampleForm{0, resample_segment_outputs(ratio, sinc_len), kResLanes};
}

hipError_t launch_resample(const double *in, double *out, const ResamplePos *pos, const double *table, int64_t n_in,
                           int64_t n_out, int64_t in_stride, int64_t out_stride, int32_t n_streams, int32_t sinc_len,
                           double ratio, int variant, hipStream_t stream) {
  ResampleArgs a{in, out, pos, table, n_in, n_out, in_stride, out_stride, n_streams, sinc_len, kResMaxRows};
  if (n_out <= 0 || n_streams <= 0) return hipSuccess;
  const ResampleForm f = resample_pick_form(ratio, sinc_len, variant);
  if (f.form == 1) return f.streams_per_workgroup == 32 ? launch_resample_mfma_variant<2>(a, stream) : launch_resample_mfma_variant<4>(a, stream);
  switch (f.segment_outputs) {
    case 128: return launch_resample_variant<16, 8>(a, stream);
    case 64: return launch_resample_variant<16, 4>(a, stream);
    case 32: return launch_resample_variant<16, 2>(a, stream);
    case 16: return launch_resample_variant<8, 2>(a, stream);
    case 8: return launch_resample_variant<4, 2>(a, stream);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace af
