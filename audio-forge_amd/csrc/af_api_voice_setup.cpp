// af_api_voice_setup.cpp -- the C ABI of the voice-chain recommendation (af_voice_setup_*): the rules of
// python/mic_eq/analysis/voice_setup.py:1143-1223 and :468-696.  Host only: no kernel and no HIP call.  The arithmetic is
// af_voice_setup_math.h's; this file checks the arguments.
#include <cmath>

#include "af_api_internal.hpp"
#include "af_voice_setup_math.h"

extern "C" {

void af_voice_setup_default_inputs(af_voice_setup_inputs *in) {
  if (in) vsm_default_inputs(in);
}

int af_voice_setup_recommend(const af_voice_setup_inputs *in, af_voice_setup_recommendation *out) {
  if (!in || !out) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  if (!in->features || !in->frame_db || !in->active_frame_mask) return fail(AF_ERR_INVALID_ARGUMENT, "features, frame_db and active_frame_mask are required");
  if (in->features->non_finite) return fail(AF_ERR_NON_FINITE, "the stream's speech features are marked non_finite");
  if (in->features->frames <= 0) return fail(AF_ERR_INVALID_ARGUMENT, "features->frames must be positive");
  if (!in->freqs || !in->spectrum_db || in->bins <= 0) return fail(AF_ERR_INVALID_ARGUMENT, "a smoothed spectrum of at least one bin is required");
  if (in->noise_status < AF_NOISE_STATUS_USABLE || in->noise_status > AF_NOISE_STATUS_INVALID)
    return fail(AF_ERR_INVALID_ARGUMENT, "noise_status must be one of AF_NOISE_STATUS_*");
  const double scalars[] = {in->residual_confidence,   in->snr_db,          in->noise_quality_score,  in->conservative_noise_rms_db,
                            in->target_lufs,           in->custom_target_p95_db, in->custom_peak_cap_db, in->enable_probability_threshold};
  for (double v : scalars)
    if (!std::isfinite(v)) return fail(AF_ERR_INVALID_ARGUMENT, "every scalar input must be finite");
  vsm_recommend(in, out);
  return AF_OK;
}

}  // extern "C"
