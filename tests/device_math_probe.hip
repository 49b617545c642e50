// Test-only probe: the device math of af_dsp.h, evaluated on the GPU over host arrays, so that tests/test_gpu_device_math.py
// can hold each helper against a high-precision reference.  Built by audio-forge_amd/csrc/Makefile with the library's
// CXXFLAGS (-ffp-contract=off: the same code the kernels run), into its own shared object.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "af_dsp.h"

namespace {

enum Fn : int32_t {
  kLog10 = 0,     // fast_log10_pos(x)
  kExp10 = 1,     // exp10(x), the call inside db2lin
  kDivKnown = 2,  // div_known(x, 20.0, 0.05)
  kDb2Lin = 3,    // db2lin(x)
  kF1 = 4,        // the gated pre-pass's F1 step: db2lin(-clamp((thr - lin2db(sqrt(x), 1e-10)) * 0.75, 0, 36))
  kF1Level = 5,   // its level: lin2db(sqrt(x), 1e-10)
};

__global__ void probe_kernel(int32_t fn, const double *in, double *out, int64_t n, double thr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x = in[i];
  double y = 0.0;
  switch (fn) {
    case kLog10: y = af::fast_log10_pos(x); break;
    case kExp10: y = exp10(x); break;
    case kDivKnown: y = af::div_known(x, 20.0, 0.05); break;
    case kDb2Lin: y = af::db2lin(x); break;
    case kF1: {  // as in supp_prefilter_gate_kernel
      const double level = af::lin2db(sqrt(x), 1e-10);
      const double d = af::dclamp((thr - level) * (1.0 - 1.0 / 4.0), 0.0, 36.0);
      y = af::db2lin(-d);
      break;
    }
    case kF1Level: y = af::lin2db(sqrt(x), 1e-10); break;
    default: y = 0.0;
  }
  out[i] = y;
}

}  // namespace

// Evaluates function `fn` on n host doubles (in -> out).  Returns 0, or the hipError_t of the first failing call.
extern "C" int af_probe_eval(int32_t fn, const double *in, double *out, int64_t n, double thr) {
  if (n <= 0) return 0;
  double *d_in = nullptr, *d_out = nullptr;
  hipError_t err = hipMalloc(&d_in, sizeof(double) * n);
  if (err == hipSuccess) err = hipMalloc(&d_out, sizeof(double) * n);
  if (err == hipSuccess) err = hipMemcpy(d_in, in, sizeof(double) * n, hipMemcpyHostToDevice);
  if (err == hipSuccess) {
    const int threads = 256;
    const int64_t blocks = (n + threads - 1) / threads;
    hipLaunchKernelGGL(probe_kernel, dim3((unsigned)blocks), dim3(threads), 0, nullptr, fn, d_in, d_out, n, thr);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err == hipSuccess) err = hipMemcpy(out, d_out, sizeof(double) * n, hipMemcpyDeviceToHost);
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  return (int)err;
}
