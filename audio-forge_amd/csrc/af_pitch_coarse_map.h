// The index map of the pitch search's coarse correlation on the matrix cores (supp_pitchsearch4_kernel, af_rnnoise.hip).
//
// xcorr[lag] = sum_{j < 240} x[j] y[j + lag] over the 147 coarse lags, x = y + 192 (the 4x-decimated whitened buffer, 432 words).
// Write lag = 16 i + c: row i = 0 .. 9 of the 16 x 16 tile, column c = 0 .. 15, and let step s = 0 .. 63 of a chain of
// v_mfma_f32_16x16x4_f32 carry, in its slot k = 0 .. 3,
//   A[i][k] = y[4 s + k + 16 i]        B[k][c] = x[4 s + k - c]   (0 where that index is outside [0, 240)).
// Then j = 4 s + k - c runs over 0 .. 239 for every column within the 64 steps, in ascending order for every (i, c): one fused
// multiply-add per term, the order of the CPU restatement's inner_prod_fma.  (With the large stride on the x side -- lag = i + 16 c,
// the first matrix form -- the columns were skewed 16 samples apart and the chain took 96 steps, more than a third of its
// products structural zeros.)
//
// Operands in LDS:
//   A  y[m] at word m + (m >> 4) of a 458-word array: one pad word per sixteen, so the sixteen rows of a step are 17 words apart
//      and the distinct words a step reads lie in distinct banks.  The largest index read is 4 x 63 + 3 + 16 x 9 = 399.  The rows
//      10 .. 15 of the tile are idle (their results are never stored): they read row 9's words, which stays inside the array and
//      adds no address to the step.
//   B  x[j] at word 15 + j of a 271-word array: 15 zero words below the data (j = -15 .. -1) and 16 above (j = 240 .. 255).
// Lane l of the wave supplies A[l & 15][l >> 4] and B[l >> 4][l & 15] and receives D[4 (l >> 4) + r][l & 15] in accumulator r.
//
// Plain constexpr functions, host and device: tests/host/pitch_coarse_map_main.cpp enumerates all 64 steps x 64 lanes.
#pragma once

namespace af {
namespace pitch_coarse {

constexpr int kSteps = 64;       // matrix instructions of the chain
constexpr int kLen = 240;        // products per lag
constexpr int kLags = 147;       // coarse lags
constexpr int kRows = 10;        // rows of the tile that hold lags (row 9: the lags 144 .. 146)
constexpr int kYLen = 432;       // words of y
constexpr int kXGuardLo = 15;    // zero words below x[0]
constexpr int kXGuardHi = 16;    // zero words above x[239]
constexpr int kXWords = kXGuardLo + kLen + kXGuardHi;  // 271

constexpr int y_word(int m) { return m + (m >> 4); }   // word of y[m] in the padded array
constexpr int kYWords = y_word(kYLen - 1) + 1;         // 458

constexpr int lane_row(int lane) { return lane & 15; }   // A's row / B's and D's column
constexpr int lane_k(int lane) { return lane >> 4; }     // the k slot the lane supplies
constexpr int used_row(int row) { return row < kRows ? row : kRows - 1; }

// the samples a slot carries
constexpr int y_index(int step, int k, int row) { return 4 * step + k + 16 * used_row(row); }
constexpr int x_index(int step, int k, int col) { return 4 * step + k - col; }  // outside [0, kLen): a guard word

// the LDS words, as a per-lane base plus a per-step offset (a compile-time constant in the written-out chain):
// y_word(4 s + k + 16 i) = 17 i + k + 4 s + (s >> 2) because k < 4 and 16 divides 16 i
constexpr int a_base(int k, int row) { return 17 * used_row(row) + k; }
constexpr int a_step(int step) { return 4 * step + (step >> 2); }
constexpr int a_word(int step, int k, int row) { return a_base(k, row) + a_step(step); }
constexpr int b_base(int k, int col) { return kXGuardLo + k - col; }
constexpr int b_step(int step) { return 4 * step; }
constexpr int b_word(int step, int k, int col) { return b_base(k, col) + b_step(step); }

// accumulator r of a lane: row 4 (lane >> 4) + r, column lane & 15
constexpr int out_row(int lane, int r) { return 4 * (lane >> 4) + r; }
constexpr int out_lag(int lane, int r) { return 16 * out_row(lane, r) + (lane & 15); }  // stored when out_row < kRows and < kLags

static_assert(a_word(kSteps - 1, 3, kRows - 1) == y_word(4 * (kSteps - 1) + 3 + 16 * (kRows - 1)), "the padded word of the largest y index");
static_assert(a_word(kSteps - 1, 3, 15) < kYWords && b_word(kSteps - 1, 3, 0) == kXWords - 1 && b_word(0, 0, 15) == 0, "operand ranges");

}  // namespace pitch_coarse
}  // namespace af
