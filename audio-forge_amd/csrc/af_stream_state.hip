// af_stream_state.hip -- the per-stream lifecycle's three kernels: restart, export (gather) and import (scatter) of a list
// of streams of a started engine, each ONE launch on the caller's stream between two process calls.  Layout, canonical ring
// and geometry: af_stream_state.h.  No chain, suppressor or pre-pass kernel knows about any of this: they find the rows they
// load at the start of their next launch as if they had left them there themselves.
#include <hip/hip_runtime.h>

#include "af_stream_state_host.hpp"
#include "af_suppressor.h"

namespace af {
namespace sstate {

static_assert(kSuppRowFloats == SuppState::kCount && kGateRowWords == kGateFields &&
                  kSuppStrengthField == SuppState::kSmoothedStrength,
              "af_stream_state.h restates the row sizes of af_suppressor.h");

namespace {

// Which piece of a region-A / region-C workgroup this thread is: `row` and the list entry `i` (A), or the entry and the
// field (C).  Every index a kernel forms from them is checked against the view before it is used.
struct Where {
  int region;  // 0 A, 1 B, 2 C, -1 nothing to do
  int row, i, field;
};
__device__ inline Where where(const Geometry &g, int32_t n) {
  Where w{-1, 0, 0, 0};
  int64_t b = blockIdx.x;
  if (b < g.a_blocks) {
    w.row = (int)(b / g.chunks);
    w.i = (int)(b % g.chunks) * kBlock + (int)threadIdx.x;
    w.region = w.i < n ? 0 : -1;
    return w;
  }
  b -= g.a_blocks;
  if (b < g.b_blocks) {
    w.i = (int)b * kBlock + (int)threadIdx.x;
    w.region = w.i < n ? 1 : -1;
    return w;
  }
  b -= g.b_blocks;
  if (b < g.c_blocks) {
    w.i = (int)(b / g.c_per_entry);
    w.field = (int)(b % g.c_per_entry) * kBlock + (int)threadIdx.x;
    w.region = (w.i < n && w.field < kSuppRowFloats) ? 2 : -1;
  }
  return w;
}

__device__ inline bool slot_ok(const PlaneView &v, const Slot &sl) {
  return (uint32_t)sl.stream < (uint32_t)v.n_streams && sl.W >= 1 && sl.W <= v.ring_cap && (uint32_t)sl.phase < (uint32_t)sl.W;
}

// ---- restart: the listed streams' columns := their preset's prototype column, gate row := 0, suppressor row := its
// initial row.  Region A covers rows64 + gate rows + EVERY f32 row (ring and suffix rows restart as zeros).
__global__ __launch_bounds__(kBlock) void stream_restart_kernel(RestartArgs a) {
  const Where w = where(a.g, a.n);
  if (w.region < 0) return;
  const Slot sl = a.slots[w.i];
  if (!slot_ok(a.v, sl) || (uint32_t)sl.preset >= (uint32_t)a.n_presets) return;
  const int64_t NS = a.v.n_streams;
  if (w.region == 2) {
    a.v.supp[(int64_t)sl.stream * kSuppRowFloats + w.field] = w.field == kSuppStrengthField ? 1.0f : 0.0f;  // rnnoise.rs:59
    return;
  }
  int r = w.row;
  if (r < a.v.rows64) {
    a.v.st64[(int64_t)r * NS + sl.stream] = a.proto64[(int64_t)sl.preset * a.v.rows64 + r];
    return;
  }
  r -= a.v.rows64;
  if (a.v.gate) {
    if (r < kGateRowWords) {
      a.v.gate[(int64_t)r * NS + sl.stream] = 0;  // NoiseGate::reset, gate.rs:759-785
      return;
    }
    r -= kGateRowWords;
  }
  if (r < a.v.rows32_plane) a.v.st32[(int64_t)r * NS + sl.stream] = r < kF32Fixed ? a.proto32[sl.preset * kF32Fixed + r] : 0.0f;
}

// ---- export: gather into the field-major staging buffer.  Region A covers the 8-byte rows and the blob's f32 rows: the
// fixed ones as they are (the prefix maximum as 0), then the ring read oldest first.
__global__ __launch_bounds__(kBlock) void stream_export_kernel(TransferArgs a) {
  const Where w = where(a.g, a.n);
  if (w.region < 0) return;
  const Slot sl = a.slots[w.i];
  if (!slot_ok(a.v, sl)) return;
  const int64_t NS = a.v.n_streams, n = a.n;
  if (w.region == 2) {
    a.stage_supp[(int64_t)w.i * kSuppRowFloats + w.field] = a.v.supp[(int64_t)sl.stream * kSuppRowFloats + w.field];
    return;
  }
  int r = w.row;
  if (r < a.v.rows64) {
    a.stage64[(int64_t)r * n + w.i] = __double_as_longlong(a.v.st64[(int64_t)r * NS + sl.stream]);
    return;
  }
  if (r < a.words64) {  // (only with a gate plane)
    a.stage64[(int64_t)r * n + w.i] = a.v.gate[(int64_t)(r - a.v.rows64) * NS + sl.stream];
    return;
  }
  r -= a.words64;
  if (r >= a.rows32) return;
  float x = 0.0f;
  if (r < kF32Fixed) {
    if (r != kLimPrefix) x = a.v.st32[(int64_t)r * NS + sl.stream];
  } else if (r - kF32Fixed < sl.W) {
    x = a.v.st32[(int64_t)(kLimRing + ring_row(sl.W, sl.phase, r - kF32Fixed)) * NS + sl.stream];
  }
  a.stage32[(int64_t)r * n + w.i] = x;
}

// ---- import: scatter from the staging buffer.  Region A covers the 8-byte rows and the fixed f32 rows but the prefix
// maximum; region B walks each entry's canonical ring into place at this engine's phase and recomputes the maxima.
__global__ __launch_bounds__(kBlock) void stream_import_kernel(TransferArgs a) {
  const Where w = where(a.g, a.n);
  if (w.region < 0) return;
  const Slot sl = a.slots[w.i];
  if (!slot_ok(a.v, sl)) return;
  const int64_t NS = a.v.n_streams, n = a.n;
  const int s = sl.stream;
  if (w.region == 2) {
    a.v.supp[(int64_t)s * kSuppRowFloats + w.field] = a.stage_supp[(int64_t)w.i * kSuppRowFloats + w.field];
    return;
  }
  if (w.region == 1) {
    const float *canon = a.stage32 + (int64_t)kF32Fixed * n + w.i;
    float *ring = a.v.st32 + (int64_t)kLimRing * NS + s;
    float *suffix = ring + (int64_t)sl.W * NS;
    const float prefix = place_ring(
        sl.W, sl.phase, [&](int c) { return canon[(int64_t)c * n]; }, [&](int row, float x) { ring[(int64_t)row * NS] = x; },
        [&](int row, float m) { suffix[(int64_t)row * NS] = m; });
    a.v.st32[(int64_t)kLimPrefix * NS + s] = prefix;
    return;
  }
  int r = w.row;
  if (r < a.v.rows64) {
    a.v.st64[(int64_t)r * NS + s] = __longlong_as_double(a.stage64[(int64_t)r * n + w.i]);
    return;
  }
  if (r < a.words64) {
    a.v.gate[(int64_t)(r - a.v.rows64) * NS + s] = a.stage64[(int64_t)r * n + w.i];
    return;
  }
  r -= a.words64;
  if (r < kF32Fixed && r != kLimPrefix) a.v.st32[(int64_t)r * NS + s] = a.stage32[(int64_t)r * n + w.i];
}

bool view_ok(const PlaneView &v) {
  return v.st64 && v.st32 && v.n_streams > 0 && v.rows64 > 0 && v.ring_cap >= 1 && v.rows32_plane == kF32Fixed + 2 * v.ring_cap;
}

}  // namespace

hipError_t launch_restart(RestartArgs a, hipStream_t stream) {
  if (a.n <= 0) return hipSuccess;
  if (!view_ok(a.v) || !a.slots || !a.proto64 || !a.proto32 || a.n_presets <= 0) return hipErrorInvalidValue;
  a.g = geometry(a.n, a.v.rows64 + (a.v.gate ? kGateRowWords : 0) + a.v.rows32_plane, false, a.v.supp != nullptr);
  hipLaunchKernelGGL(stream_restart_kernel, dim3((unsigned)a.g.total()), dim3(kBlock), 0, stream, a);
  return hipGetLastError();
}

static bool transfer_ok(const TransferArgs &a) {
  return view_ok(a.v) && a.slots && a.stage64 && a.stage32 && a.words64 == a.v.rows64 + (a.v.gate ? kGateRowWords : 0) &&
         a.rows32 == kF32Fixed + a.v.ring_cap && (a.v.supp == nullptr) == (a.stage_supp == nullptr);
}

hipError_t launch_export(TransferArgs a, hipStream_t stream) {
  if (a.n <= 0) return hipSuccess;
  if (!transfer_ok(a)) return hipErrorInvalidValue;
  a.g = geometry(a.n, a.words64 + a.rows32, false, a.v.supp != nullptr);
  hipLaunchKernelGGL(stream_export_kernel, dim3((unsigned)a.g.total()), dim3(kBlock), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_import(TransferArgs a, hipStream_t stream) {
  if (a.n <= 0) return hipSuccess;
  if (!transfer_ok(a)) return hipErrorInvalidValue;
  a.g = geometry(a.n, a.words64 + kF32Fixed, true, a.v.supp != nullptr);
  hipLaunchKernelGGL(stream_import_kernel, dim3((unsigned)a.g.total()), dim3(kBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace sstate
}  // namespace af
