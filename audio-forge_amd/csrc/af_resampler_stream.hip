// af_resampler_stream.hip -- the product resampler as the realtime loop runs it (rust-core/src/audio/processor/
// dsp_loop.rs:274-317, 843-895, 963-1011): a SincFixedIn that lives across calls, fed f32, drained as f32.
//
// State plane.  Per stream one f32 row of 2 * sinc_len + chunk - 1 frames: [ history: the last 2 * sinc_len frames the
// resampler has consumed | the frames queued behind them that do not fill a chunk yet ].  The inputs are f32, so keeping
// them as f32 loses nothing; the crate's f64 buffer holds the same values widened.
//
// Virtual input axis.  A call that completes k chunks reads "plane, then this call's input" as one axis:
//   v in [0, split)            -> plane[v]               split = 2 * sinc_len + frames pending before the call
//   v in [split, split + n_in) -> in[v - split]
// Chunk j's buffer (the crate's [2 * sinc_len history | chunk]) starts at v = j * chunk, so the host's position records
// (af_resampler_host.hpp: chunk_positions with origin j * chunk + 2 * sinc_len) address the axis directly and are never
// negative.  The load role widens f32 -> f64 (exact) on the way into LDS, the store role rounds f64 -> f32 to nearest even
// (the loop's `sample as f32`); everything in between is the one-shot kernels' own body (af_resampler_body.h): same tiles,
// same fused multiply-add chains, same cubic, matrix-core form where resample_mfma_ok holds and the vector form elsewhere.
//
// Advancing the plane.  The plane is a ping-pong pair.  After the resampling launch, in stream order, a small kernel writes
// the OTHER plane: next[i] = axis[k * chunk + i] for i < 2 * sinc_len + remainder.  No workgroup reads a row another one
// has written in the same call: the resampling launch and the advance launch both read the current plane only.
#include <hip/hip_runtime.h>

#include "af_resampler_body.h"

namespace af {

struct ResampleStreamArgs {
  const float *plane;       // [n_streams][plane_stride], the current one of the pair
  const float *in;          // [n_streams][in_stride], this call's frames
  float *out;               // [n_streams][out_stride]
  const ResamplePos *pos;   // [n_out], on the virtual axis
  const double *table;
  int64_t split, n_axis;    // frames of the axis that come from the plane; frames of the axis in all (split + n_in)
  int64_t n_out, in_stride, out_stride;
  int32_t plane_stride, n_streams, sinc_len, max_rows;
};

struct ResampleIoStream {
  const float *plane, *in;
  float *out;
  int64_t split, n_axis, in_stride, out_stride;
  int32_t plane_stride;
  struct InRow {
    const float *hist, *cur;  // cur is biased by -split: cur[v] is valid for v in [split, n_axis)
    int64_t split, n_axis;
    __device__ __forceinline__ double at(int64_t v) const {
      if (v < 0 || v >= n_axis) return 0.0;  // only the zero pad taps of a tile's round-up reach past the axis
      return (double)(v < split ? hist[v] : cur[v]);
    }
  };
  struct OutRow {
    float *dst;
    __device__ __forceinline__ void put(int64_t o, double v) const { dst[o] = (float)v; }  // v_cvt_f32_f64: nearest even
  };
  __device__ __forceinline__ InRow in_row(int s) const {
    return InRow{plane + (int64_t)s * plane_stride, in + (int64_t)s * in_stride - split, split, n_axis};
  }
  __device__ __forceinline__ OutRow out_row(int s) const { return OutRow{out + (int64_t)s * out_stride}; }
};

__device__ __forceinline__ ResampleCore stream_core(const ResampleStreamArgs &a) {
  return ResampleCore{a.pos, a.table, a.n_out, a.n_streams, a.sinc_len, a.max_rows};
}
__device__ __forceinline__ ResampleIoStream stream_io(const ResampleStreamArgs &a) {
  return ResampleIoStream{a.plane, a.in, a.out, a.split, a.n_axis, a.in_stride, a.out_stride, a.plane_stride};
}

template <int kWaves, int kOutPerWave>
__global__ __launch_bounds__(kWaves *kResLanes) void resample_stream_kernel(ResampleStreamArgs a) {
  extern __shared__ double lds[];  // [max(rows, segment outputs)][65]
  resample_valu_body<kWaves, kOutPerWave>(stream_core(a), stream_io(a), lds);
}

template <int kGroups>
__global__ __launch_bounds__(kGroups * 4 * kResLanes) void resample_stream_mfma_kernel(ResampleStreamArgs a) {
  extern __shared__ double lds[];  // [kGroups][kMfRows][16 streams]; later [128 outputs][kStreams + 1]
  resample_mfma_body<kGroups>(stream_core(a), stream_io(a), lds);
}

// next[s][i] = axis[s][shift + i], i < count (= 2 * sinc_len + the call's remainder <= plane_stride)
__global__ __launch_bounds__(256) void resample_stream_advance_kernel(const float *plane, float *next, const float *in, int64_t split,
                                                                       int64_t shift, int64_t in_stride, int32_t count,
                                                                       int32_t plane_stride, int32_t n_streams) {
  const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int s = (int)(cell / count), i = (int)(cell % count);
  if (s >= n_streams) return;
  const int64_t v = shift + i;
  next[(int64_t)s * plane_stride + i] = v < split ? plane[(int64_t)s * plane_stride + v] : in[(int64_t)s * in_stride + (v - split)];
}

template <int kGroups>
static hipError_t launch_stream_mfma(const ResampleStreamArgs &a, hipStream_t stream) {
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(resample_stream_mfma_kernel<kGroups>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (err != hipSuccess) return err;
    attr_set = true;
  }
  const size_t dyn = sizeof(double) * kGroups * kMfRows * 16;
  const dim3 grid((unsigned)((a.n_out + kMfSeg - 1) / kMfSeg), (unsigned)((a.n_streams + 16 * kGroups - 1) / (16 * kGroups)));
  hipLaunchKernelGGL(resample_stream_mfma_kernel<kGroups>, grid, dim3(kGroups * 4 * kResLanes), dyn, stream, a);
  return hipGetLastError();
}

template <int kWaves, int kOutPerWave>
static hipError_t launch_stream_valu(const ResampleStreamArgs &a, hipStream_t stream) {
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(resample_stream_kernel<kWaves, kOutPerWave>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (err != hipSuccess) return err;
    attr_set = true;
  }
  constexpr int kSeg = kWaves * kOutPerWave;
  const size_t dyn = sizeof(double) * kResRowStride * (size_t)kResMaxRows;
  const dim3 grid((unsigned)((a.n_out + kSeg - 1) / kSeg), (unsigned)((a.n_streams + kResLanes - 1) / kResLanes));
  hipLaunchKernelGGL((resample_stream_kernel<kWaves, kOutPerWave>), grid, dim3(kWaves * kResLanes), dyn, stream, a);
  return hipGetLastError();
}

// The chunks a call completes: n_out frames per stream from the axis (plane | in).  variant as launch_resample.
hipError_t launch_resample_stream(const float *plane, const float *in, float *out, const ResamplePos *pos, const double *table,
                                  int64_t split, int64_t n_in, int64_t n_out, int64_t in_stride, int64_t out_stride,
                                  int32_t plane_stride, int32_t n_streams, int32_t sinc_len, double ratio, int variant,
                                  hipStream_t stream) {
  if (n_out <= 0 || n_streams <= 0) return hipSuccess;
  if (split < 0 || split > plane_stride || n_in < 0) return hipErrorInvalidValue;
  ResampleStreamArgs a{plane, in, out, pos, table, split, split + n_in, n_out, in_stride, out_stride, plane_stride, n_streams,
                       sinc_len, kResMaxRows};
  const ResampleForm f = resample_pick_form(ratio, sinc_len, variant);
  if (f.form == 1) return f.streams_per_workgroup == 32 ? launch_stream_mfma<2>(a, stream) : launch_stream_mfma<4>(a, stream);
  switch (f.segment_outputs) {
    case 128: return launch_stream_valu<16, 8>(a, stream);
    case 64: return launch_stream_valu<16, 4>(a, stream);
    case 32: return launch_stream_valu<16, 2>(a, stream);
    case 16: return launch_stream_valu<8, 2>(a, stream);
    case 8: return launch_stream_valu<4, 2>(a, stream);
    default: return hipErrorInvalidValue;
  }
}

// The plane of the next call: `count` frames of the axis from `shift` on (see the file comment).
hipError_t launch_resample_stream_advance(const float *plane, float *next, const float *in, int64_t split, int64_t n_in,
                                          int64_t shift, int64_t in_stride, int32_t count, int32_t plane_stride, int32_t n_streams,
                                          hipStream_t stream) {
  if (count <= 0 || n_streams <= 0) return hipSuccess;
  if (count > plane_stride || shift < 0 || shift + count > split + n_in || split > plane_stride) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(((int64_t)count * n_streams + 255) / 256));
  hipLaunchKernelGGL(resample_stream_advance_kernel, grid, dim3(256), 0, stream, plane, next, in, split, shift, in_stride, count,
                     plane_stride, n_streams);
  return hipGetLastError();
}

}  // namespace af
