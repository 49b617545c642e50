/* compressor_search_ref.c -- the CPU side of tests/test_compressor_search_ref.py: the calibration search, the fold of a
 * simulation's block rows and the per-capture masks of csrc/af_compressor_search_math.h (the header the library's host half includes) behind a C interface a test can
 * drive step by step, with the simulations answered by the CPU oracle.  Built by tests/compressor_search_oracle.py. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../audio-forge_amd/csrc/af_compressor_search_math.h"

csm_search *csr_new(const csm_settings *settings) {
  csm_search *s = (csm_search *)malloc(sizeof *s);
  if (s) csm_begin(s, settings);
  return s;
}

void csr_free(csm_search *s) { free(s); }

int csr_phase1(csm_search *s) { return csm_phase1(s); }

int csr_phase2(csm_search *s) { return csm_phase2(s); }

/* the clamped values of the entries that wait for a simulation, [count][4]; returns count */
int csr_waiting(const csm_search *s, double *values) {
  for (int i = s->n_scored; i < s->n; ++i) memcpy(values + (size_t)(i - s->n_scored) * CSM_CONTROLS, s->entries[i].values, sizeof(double) * CSM_CONTROLS);
  return s->n - s->n_scored;
}

void csr_score(csm_search *s, const csm_simulation *sims, int count) {
  for (int i = 0; i < count; ++i) csm_score(s, &sims[i]);
}

void csr_choose(const csm_search *s, csm_choice *out) { csm_choose(s, out); }

/* every scored entry in evaluation order: values [n][4], scores [n]; returns n */
int csr_entries(const csm_search *s, double *values, double *scores) {
  for (int i = 0; i < s->n_scored; ++i) {
    memcpy(values + (size_t)i * CSM_CONTROLS, s->entries[i].values, sizeof(double) * CSM_CONTROLS);
    scores[i] = s->entries[i].score;
  }
  return s->n_scored;
}

int csr_capture_masks(const double *input_square_sum, int n_blocks, int64_t n_samples, int control_block, float *in_db, uint8_t *mask,
                      float *active_threshold_db) {
  float *scratch = (float *)malloc(sizeof(float) * (size_t)(n_blocks > 0 ? n_blocks : 1));
  if (!scratch) return -1;
  const int active = csm_capture_masks(input_square_sum, 1, n_blocks, n_samples, control_block, in_db, mask, scratch, active_threshold_db);
  free(scratch);
  return active;
}

void csr_pumping_alphas(float cadence_hz, float *highpass_alpha, float *lowpass_alpha) { csm_pumping_alphas(cadence_hz, highpass_alpha, lowpass_alpha); }

double csr_round6(double x) { return csm_round6(x); }

/* the fold of one simulation's rows (csm_fold); returns -1 when it cannot allocate */
int csr_fold(const csm_fold_rows *rows, int n_blocks, int64_t n_samples, int control_block, float ceiling_db, csm_fold_result *out) {
  const size_t n = (size_t)(n_blocks > 0 ? n_blocks : 1);
  float *scratch = (float *)malloc(sizeof(float) * 6 * n);
  uint8_t *bytes = (uint8_t *)malloc(2 * n);
  if (scratch && bytes) csm_fold(rows, n_blocks, n_samples, control_block, ceiling_db, out, scratch, bytes);
  const int rc = scratch && bytes ? 0 : -1;
  free(scratch);
  free(bytes);
  return rc;
}
