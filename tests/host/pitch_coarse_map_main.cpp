// The index map of the pitch search's coarse correlation (csrc/af_pitch_coarse_map.h), enumerated over all 64 steps x 64 lanes
// of the matrix chain against the sum it stands for -- xcorr[lag] = sum_{j < 240} x[j] y[j + lag], 147 lags -- with the two LDS
// arrays modelled as the kernel fills them.  Stand-alone host program (no GPU, no HIP runtime), built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_host_pitch_coarse_map.py.
//
// Checked:
//   1. every (lag < 147, j < 240) pair is visited exactly once, with j ascending per lag (steps in order, k = 0 .. 3 inside a step),
//      and the y sample that meets x[j] is y[j + lag];
//   2. every A and B word lies inside its array, the idle rows 10 .. 15 included (the arrays are heap blocks of exactly the
//      map's sizes: the sanitizer sees a stray read as well);
//   3. a guard word of B is read exactly where j is outside [0, 240), and holds zero; a pad word of A is never read;
//   4. within a step no two lanes that read DIFFERENT words meet in one bank -- for A and for B, in both banking models of a
//      one-word LDS read (the wave as two groups of 32 lanes over 32 banks; all 64 lanes over 64 banks).  Lanes that read the
//      same word are one broadcast access: a step reads 40 distinct A words (10 rows x 4 slots) and 19 distinct B words, so
//      "64 distinct banks" can only mean this;
//   5. the per-lane base + per-step offset form the kernel uses equals the padded word of the sample index;
//   6. the accumulators of the lanes cover the lags 0 .. 146 exactly once.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "af_pitch_coarse_map.h"

namespace cm = af::pitch_coarse;

static int failures = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      if (++failures <= 20) {                     \
        std::printf("FAIL %s: ", #cond);          \
        std::printf(__VA_ARGS__);                 \
        std::printf("\n");                        \
      }                                           \
    }                                             \
  } while (0)

int main() {
  // the arrays as the kernel fills them: y[m] = m + 1 (never zero), x = y + 192; pads marked, guards zero
  const double kPad = -12345.0;
  std::vector<double> ya(cm::kYWords, kPad), xb(cm::kXWords, 0.0);
  std::vector<int> y_of_word(cm::kYWords, -1);
  for (int m = 0; m < cm::kYLen; ++m) {
    CHECK(cm::y_word(m) >= 0 && cm::y_word(m) < cm::kYWords && y_of_word[cm::y_word(m)] == -1, "y word of %d", m);
    ya[cm::y_word(m)] = m + 1.0;
    y_of_word[cm::y_word(m)] = m;
  }
  for (int j = 0; j < cm::kLen; ++j) xb[cm::kXGuardLo + j] = (cm::kYLen - cm::kLen) + j + 1.0;

  std::vector<int> visits(cm::kLags * cm::kLen, 0), last_j(cm::kLags, -1);
  for (int step = 0; step < cm::kSteps; ++step) {
    int a_words[64], b_words[64];
    for (int lane = 0; lane < 64; ++lane) {
      const int k = cm::lane_k(lane), rc = cm::lane_row(lane);
      const int aw = cm::a_word(step, k, rc), bw = cm::b_word(step, k, rc);
      a_words[lane] = aw;
      b_words[lane] = bw;
      CHECK(aw >= 0 && aw < cm::kYWords, "A word %d at step %d lane %d", aw, step, lane);
      CHECK(bw >= 0 && bw < cm::kXWords, "B word %d at step %d lane %d", bw, step, lane);
      if (aw < 0 || aw >= cm::kYWords || bw < 0 || bw >= cm::kXWords) continue;
      const double av = ya[aw], bv = xb[bw];  // (the sanitizer's view of the same reads)
      CHECK(av != kPad && y_of_word[aw] == cm::y_index(step, k, rc), "A reads y[%d] for y[%d]", y_of_word[aw], cm::y_index(step, k, rc));
      CHECK(aw == cm::y_word(cm::y_index(step, k, rc)), "base + offset form of A at step %d lane %d", step, lane);
      const int j = cm::x_index(step, k, rc);
      CHECK(bw == cm::kXGuardLo + j, "base + offset form of B at step %d lane %d", step, lane);
      const bool guard = bw < cm::kXGuardLo || bw >= cm::kXGuardLo + cm::kLen;
      CHECK(guard == (j < 0 || j >= cm::kLen), "guard word at j = %d", j);
      CHECK(!guard || bv == 0.0, "guard word holds %g", bv);
      CHECK(guard || bv == (cm::kYLen - cm::kLen) + j + 1.0, "B reads %g for x[%d]", bv, j);
    }
    // the products of this step: D[i][c] += A[i][k] B[k][c] for k = 0 .. 3 in order; lane (k, i) supplies A, lane (k, c) supplies B
    for (int i = 0; i < 16; ++i)
      for (int c = 0; c < 16; ++c)
        for (int k = 0; k < 4; ++k) {
          const int j = cm::x_index(step, k, c), lag = 16 * i + c;
          if (i >= cm::kRows || lag >= cm::kLags || j < 0 || j >= cm::kLen) continue;  // dropped row / lag, or a zero product
          CHECK(cm::y_index(step, k, i) == j + lag, "y[%d] meets x[%d] at lag %d", cm::y_index(step, k, i), j, lag);
          CHECK(j > last_j[lag], "j = %d after %d at lag %d", j, last_j[lag], lag);
          last_j[lag] = j;
          ++visits[lag * cm::kLen + j];
        }
    // banks: distinct words of one lane group in distinct banks
    for (int model = 0; model < 2; ++model) {
      const int group = model == 0 ? 32 : 64, banks = model == 0 ? 32 : 64;
      for (int g0 = 0; g0 < 64; g0 += group)
        for (int p = g0; p < g0 + group; ++p)
          for (int q = p + 1; q < g0 + group; ++q) {
            CHECK(a_words[p] == a_words[q] || a_words[p] % banks != a_words[q] % banks, "A bank conflict at step %d, lanes %d and %d (%d banks)", step, p, q, banks);
            CHECK(b_words[p] == b_words[q] || b_words[p] % banks != b_words[q] % banks, "B bank conflict at step %d, lanes %d and %d (%d banks)", step, p, q, banks);
          }
    }
  }
  for (int lag = 0; lag < cm::kLags; ++lag)
    for (int j = 0; j < cm::kLen; ++j) CHECK(visits[lag * cm::kLen + j] == 1, "(lag %d, j %d) visited %d times", lag, j, visits[lag * cm::kLen + j]);

  std::vector<int> stored(cm::kLags, 0);
  for (int lane = 0; lane < 64; ++lane)
    for (int r = 0; r < 4; ++r) {
      const int row = cm::out_row(lane, r), lag = cm::out_lag(lane, r);
      CHECK(lag == 16 * row + (lane & 15) && row >= 0 && row < 16, "accumulator %d of lane %d", r, lane);
      if (row < cm::kRows && lag < cm::kLags) ++stored[lag];
    }
  for (int lag = 0; lag < cm::kLags; ++lag) CHECK(stored[lag] == 1, "lag %d stored %d times", lag, stored[lag]);

  if (failures) {
    std::printf("pitch_coarse_map: %d failures\n", failures);
    return 1;
  }
  std::printf("pitch_coarse_map: ok (%d steps x 64 lanes, %d lags x %d products)\n", cm::kSteps, cm::kLags, cm::kLen);
  return 0;
}
