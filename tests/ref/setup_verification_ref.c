/* setup_verification_ref.c -- csrc/af_setup_verification_math.h behind a C interface, for the tests: the measurements of
 * validate_voice_setup_verification (voice_setup.py:1446-1679) on one stream, in the kernels' operation order.  The arithmetic is
 * the header's; nothing is restated here. */
#include "../../audio-forge_amd/csrc/af_setup_verification_math.h"

int svr_preset_id(const char *name) { /* get_target_curve's ValueError is the caller's: -1 */
  int p;
  for (p = 0; p < AF_TARGET_PRESET_COUNT; ++p)
    if (strcmp(name, svm_preset_names[p]) == 0) return p;
  return -1;
}

/* get_target_curve(freqs, preset, measured, "adaptive"); measured null = "static".  scalars: the nine of svm_offset_scalars */
void svr_target_curve(const double *freqs, const double *measured_db, int n, int preset, double *target, double *scalars) {
  double *work = (double *)malloc(sizeof(double) * 2 * (size_t)(n > 0 ? n : 1));
  svm_offset_scalars o;
  svm_target_curve(freqs, measured_db, n, preset, target, &o, work);
  memcpy(scalars, &o, sizeof o);
  free(work);
}

double svr_shape_error_db(const double *freqs, const double *db, int K, int preset, double *scalars /* [5] */) {
  svm_offset_scalars o;
  const double err = svm_shape_error_db(freqs, db, K, preset, &o);
  memcpy(scalars, &o, sizeof(double) * 5);
  return err;
}

double svr_repeatability_delta_db(const double *freqs, const double *before_db, int K, const double *original_freqs,
                                  const double *original_db, int K0) {
  return svm_repeatability_delta_db(freqs, before_db, K, original_freqs, original_db, K0);
}

void svr_snr_band_medians(const double *freqs, const double *snr_db, int K, double *medians, int32_t *present) {
  svm_snr_band_medians(freqs, snr_db, K, medians, present);
}

double svr_sum_squares(const float *x, int64_t n) { return svm_sum_squares(x, n); }
double svr_rms_db(double sum_squares, int64_t n) { return svm_rms_db(sum_squares, n); }

void svr_measure_row(const double *freqs, int K, const double *original_db, const double *before_db, const double *after_db,
                     const double *after_snr_db, int preset, const float *const *audio, const int64_t *lengths,
                     af_setup_verification_row *row) {
  svm_measure_row(freqs, K, original_db, before_db, after_db, after_snr_db, preset, audio, lengths, row);
}

void svr_decide(const af_setup_verification_row *row, const af_setup_verification_evidence *evidence, af_setup_verification_result *out) {
  svm_decide(row, evidence, out);
}
const char *svr_reason_text(int reason) { return reason >= 0 && reason < AF_SETUP_REASON_COUNT ? svm_reason_texts[reason] : NULL; }

void svr_offline_validation(const af_setup_offline_inputs *in, af_setup_offline_result *out) { svm_offline_validation(in, out); }
const char *svr_uncertainty_text(int bit) { return bit >= 0 && bit < AF_SETUP_UNCERTAIN_COUNT ? svm_uncertainty_texts[bit] : NULL; }
