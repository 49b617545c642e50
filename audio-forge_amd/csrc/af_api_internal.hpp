// af_api_internal.hpp -- what the translation units of the C ABI (af_api*.cpp) share: the calling thread's last-error text, the
// two ways to fail, the owner types of af_hip_resources.hpp, and the two helpers at the end.  Everything else goes through
// include/audioforge_mi.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../include/audioforge_mi.h"
#include "af_hip_resources.hpp"

// what af_last_error returns; defined in af_api.cpp
__attribute__((visibility("hidden"))) extern thread_local std::string af_last_error_text;

__attribute__((format(printf, 2, 3))) static inline int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  af_last_error_text = buf;
  return code;
}

#define AF_HIP(expr)                                                                              \
  do {                                                                                            \
    hipError_t err__ = (expr);                                                                    \
    if (err__ != hipSuccess)                                                                      \
      return fail(AF_ERR_BACKEND, "%s failed: %s", #expr, hipGetErrorString(err__));              \
  } while (0)

// The argument checks af_resampler_create and af_stream_resampler_create share; defined in af_api_resampler.cpp, not exported.
// (It sets the last-error text and returns ABI codes, so it does not belong in af_resampler_host.hpp, which device sources include.)
__attribute__((visibility("hidden"))) int af_resampler_check_arguments(uint32_t input_rate, uint32_t output_rate, int64_t chunk_size,
                                                                      int32_t sinc_len, int32_t window, int32_t device);

// What af_noise_suppressor_reset (af_api_noise_suppressor.cpp) asks of its engine; defined in af_api.cpp, not exported.  A no-op
// before streaming has started; otherwise the device comes to rest and every stream's suppressor state row is initialised
// again, except its smoothed wet/dry strength, which is kept.
__attribute__((visibility("hidden"))) int af_engine_reinit_suppressor_state(af_engine *e);
