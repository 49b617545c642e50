// af_retune.hip -- live control's state-retune kernel: the ordered edit list of the setters called since the last call,
// applied to the f64 state plane in ONE launch in front of the call's first chain kernel.
#include <hip/hip_runtime.h>

#include "af_deesser_math.h"
#include "af_retune.h"

namespace af {

// One lane per stream, one workgroup per 64-stream group.  A lane reads and writes its own column only, so program order is
// the list's order; the op list and the group's preset are wave-uniform (scalar loads), the plane accesses are coalesced
// vector loads / stores of consecutive streams.  Rows outside the plane are skipped, never written.
__global__ __launch_bounds__(kLanes) void retune_state_kernel(RetuneArgs a) {
  const int g = blockIdx.x;
  const int s = g * kLanes + threadIdx.x;
  if (s >= a.n_streams) return;
  const int preset = a.group_preset ? a.group_preset[g] : 0;
  const int64_t NS = a.n_streams;
  const uint32_t rows = (uint32_t)a.n_fields;
  for (int k = 0; k < a.n_ops; ++k) {
    const RetuneOp op = a.ops[k];
    if (op.preset != preset || (uint32_t)op.dst >= rows) continue;
    if (op.kind == kRetunePeaking) {
      if ((uint32_t)op.src >= rows || (uint32_t)op.dst + 4u >= rows) continue;
      const BiquadCoef c = deess::peaking(op.value, op.value2, a.st64[(int64_t)op.src * NS + s]);
      const double v5[5] = {c.b0, c.b1, c.b2, c.a1, c.a2};
#pragma unroll
      for (int j = 0; j < 5; ++j) a.st64[(int64_t)(op.dst + j) * NS + s] = v5[j];
      continue;
    }
    double v = op.value;
    if (op.kind == kRetuneCopy) {
      if ((uint32_t)op.src >= rows) continue;
      v = a.st64[(int64_t)op.src * NS + s];
    }
    a.st64[(int64_t)op.dst * NS + s] = v;
  }
}

hipError_t launch_retune_state(const RetuneArgs &a, hipStream_t stream) {
  if (a.n_ops <= 0 || a.n_streams <= 0) return hipSuccess;
  const int groups = (a.n_streams + kLanes - 1) / kLanes;
  hipLaunchKernelGGL(retune_state_kernel, dim3(groups), dim3(kLanes), 0, stream, a);
  return hipGetLastError();
}

}  // namespace af
