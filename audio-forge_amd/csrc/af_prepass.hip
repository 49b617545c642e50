// af_prepass.hip -- the sample-serial pre-pass in front of the chain: the realtime front end (scrub, clamp, DC block, 80 Hz
// high-pass; routing.rs:802-843), the noise gate (dsp/gate.rs, realtime stage 1) and the suppressor's model input (scaling,
// RNNoise's own high-pass, the 1728-sample history), as pipelines of wave roles over tiles of 64 streams.
//   supp_prefilter_kernel        front end + model input, no gate: the suppressor's pre-pass of a window
//   supp_prefilter_gate_kernel   front end + expander gate (+ model input); without the suppressor's roles it is the engine's
//                                gate stage
//   vad_gate_control_kernel      the VAD-fused modes' controller, once per control block
//   vad_gate_prepass_kernel      front end + VAD-fused gate (+ model input)
//   vad_plane_init_kernel        the fused modes' state plane at reset
// What the kernels share is in af_prepass.h; each kernel keeps its load role, its LDS carve-up and the loops (and unroll
// factors) of its lane = stream roles.
#include <hip/hip_runtime.h>

#include "af_prepass.h"

namespace af {

// test tap: scale_for_model, element-wise (the reference pins it in rnnoise.rs:335-352)
__global__ void supp_scale_probe_kernel(const float *in, float *out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = scale_for_model(in[i]);
}
hipError_t launch_scale_probe(const float *in, float *out, int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(supp_scale_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, in, out, n);
  return hipGetLastError();
}

// The pass is a chain of short per-sample recurrences (DC block and 80 Hz high-pass in f64; the model's own high-pass)
// around a feed-forward soft clip, so its duration is samples x (instructions on the longest recurrence) x ~8 cycles (one
// wave issues a dependent vector instruction every ~8 cycles: tools/probe/valu_latency.hip) whatever the lane count.  As one
// wave doing everything that was ~800 cycles per sample (2.4-3.0 ms per 8 880-sample window at ANY batch: what a small batch
// waited for).  Now a workgroup of six waves takes 64 streams and works as a pipeline over kPreT-sample tiles, one barrier per
// tile: wave 0 loads tile i (transposed into LDS), wave 1 runs the front end on tile i-1 IN PLACE (lane = stream), wave 2
// the soft clip of tile i-2 into a second ring (lane = TIME), wave 3 the model's high-pass on tile i-3 in place there
// (lane = stream), waves 4 and 5 write the dry signal of tile i-2 and the model input of tile i-4 back as rows.  A tile of
// either ring is in flight for three iterations, so each ring holds three.
// Tile length (AF_PRE_TILE, a power of two up to 64): 32 samples.  The six tiles are then 49 920 bytes and
// two transform workgroups, or a search workgroup and a transform workgroup, fit on the CU beside this one; eight tiles of
// 64 samples (133 120 bytes) left room for nothing but the tracker.  The lane = time roles keep all 64 lanes busy: lane l
// works on sample l % kPreT of row (l / kPreT) * kPreT + r, so a row segment is kPreT x 4 bytes (128: still a whole cache
// line) and a wave touches 64 / kPreT rows per instruction.
#ifndef AF_PRE_TILE
#define AF_PRE_TILE 32
#endif
constexpr int kPreWaves = 6;
constexpr int kPreT = AF_PRE_TILE;               // samples per tile
constexpr int kPreTile = kPreT * kPreRow;        // floats per LDS tile
constexpr int kPreRing = 3;                      // tiles per ring
constexpr bool kPreRagged = kRnnFrame % kPreT != 0;  // a window is whole frames: at 32 (480 = 15 x 32) no tile is short
static_assert(kPreT >= 8 && kPreT <= 64 && (kPreT & (kPreT - 1)) == 0, "the tile length divides the wave");
template <bool kClamp, bool kDcHp, bool kRaw>
__global__ __launch_bounds__(64 * kPreWaves) void supp_prefilter_kernel(SuppArgs a) {
  extern __shared__ float pre_lds[];  // in -> dry [3], sc -> xh [3]
  constexpr bool kFront = kClamp || kDcHp;
  constexpr int T = kPreT;
  float *t_dry = pre_lds, *t_xh = pre_lds + kPreRing * kPreTile;
  auto sel = [](int64_t ti) { return (int)(ti % kPreRing) * kPreTile; };  // (ti >= 0)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tl = lane & (T - 1), row0 = (lane / T) * T;  // lane = time roles: sample tl of rows row0 + r, r < T
  const int s0 = blockIdx.x * kPreGroup;
  const int s = s0 + lane;
  const bool valid = s < a.n_streams;
  const int sc = valid ? s : a.n_streams - 1;
  const int64_t NS = a.n_streams;
  const int64_t n = (int64_t)a.n_frames * kRnnFrame;
  const int64_t xh_stride = kPitchBuf + n;
  float *st = a.state + (int64_t)sc * SuppState::kCount;
  const int64_t ntiles = (n + T - 1) / T;
  auto at = [](float *tile, int t, int col) -> float & { return tile[t * kPreRow + col]; };
  auto len_of = [&](int64_t ti) { return kPreRagged ? tile_len<T>(n, ti) : T; };

  copy_model_history<9>(a, s0, wave, kPreWaves, lane, xh_stride);

  // per-role state
  ModelHp mhp;
  FrontEnd fe;
  if (wave == 3) mhp.load(st);
  if (wave == 1 && kDcHp) fe.load(a, NS, sc);
  const double hb0 = a.hp_b0, hb1 = a.hp_b1, hb2 = a.hp_b2, ha1 = a.hp_a1, ha2 = a.hp_a2;
  const bool hp_on = a.front_hp != 0;
  // the load wave's rows: first_row + min(r, rows_left) (clamped, not skipped: the T loads stay in flight together)
  const int first_row = (s0 + row0) < a.n_streams ? (s0 + row0) : a.n_streams - 1;
  const float *const in_lane = a.in + (int64_t)first_row * a.in_stride + a.frame0 * kRnnFrame;

  // The load wave keeps one tile in flight in registers: tile it + 1 is requested when tile `it` has gone to LDS, so the
  // loads' latency passes during the iteration before the one that needs them (what a small batch, whose pre-pass has the
  // chip to itself, waits for: at 32 samples a tile's recurrences are shorter than one load).  The T row addresses are the
  // same for every tile but for the column: left to itself the compiler keeps all of them in registers for the whole kernel
  // (64 VGPRs for every wave of it).  So the tile's first address and the row limit pass through an empty asm, and each
  // row's address is two independent adds from there -- independent: a pointer walked from row to row made the loads one
  // more recurrence.
  float v[T];
  auto request = [&](int64_t ti) {
    const int len = len_of(ti);
    const float *p = in_lane + ti * T + (tl < len ? tl : len - 1);
    int rows_left = a.n_streams - 1 - first_row;
    asm volatile("" : "+v"(p), "+v"(rows_left));
    const float *const p_last = p + (int64_t)rows_left * a.in_stride;
#pragma unroll
    for (int r = 0; r < T; ++r) v[r] = *(r <= rows_left ? p + (int64_t)r * a.in_stride : p_last);
  };
  if (wave == 0 && ntiles > 0) request(0);

  // (every wave runs every iteration and its barrier: the trip count is uniform and no role returns early)
  for (int64_t it = 0; it < ntiles + 4; ++it) {
    if (wave == 0) {  // ---- tile `it` to LDS, transposed; request tile it + 1
      const int64_t ti = it;
      if (ti < ntiles) {
        float *tile = t_dry + sel(ti);
#pragma unroll
        for (int r = 0; r < T; ++r) at(tile, tl, row0 + r) = v[r];
        if (ti + 1 < ntiles) request(ti + 1);
      }
    } else if (wave == 1) {  // ---- front end on tile it - 1, in place (lane = stream): routing.rs:802-843
      const int64_t ti = it - 1;
      if (kFront && ti >= 0 && ti < ntiles) {
        const int len = len_of(ti);
        float *tile = t_dry + sel(ti);
#pragma unroll 8
        for (int t = 0; t < T; ++t) {
          if (t < len) at(tile, t, lane) = fe.step(at(tile, t, lane), true, kClamp, kDcHp, hp_on, hb0, hb1, hb2, ha1, ha2);
        }
      }
    } else if (wave == 2) {  // ---- model-input scaling of tile it - 2 (lane = time)
      const int64_t ti = it - 2;
      if (ti >= 0 && ti < ntiles) scale_tile_for_model<kRaw, T, kPreRow, 8>(t_dry + sel(ti), t_xh + sel(ti), lane);
    } else if (wave == 3) {  // ---- the model's own high-pass on tile it - 3, in place (lane = stream)
      const int64_t ti = it - 3;
      if (ti >= 0 && ti < ntiles) {
        const int len = len_of(ti);
        float *tile = t_xh + sel(ti);
#pragma unroll 8
        for (int t = 0; t < T; ++t) {
          if (t < len) at(tile, t, lane) = mhp.step(at(tile, t, lane));
        }
      }
    } else if (wave == 4) {  // ---- the dry signal the wet/dry mix sees is the suppressor's input, i.e. the front end's output
      const int64_t ti = it - 2;
      if (kFront && ti >= 0 && ti < ntiles)
        write_tile_rows<T, kPreRow, 8>(t_dry + sel(ti), a.out + a.frame0 * kRnnFrame + ti * T, a.stream_stride, s0, a.n_streams,
                                       len_of(ti), lane);
    } else {  // ---- the model input of tile it - 4
      const int64_t ti = it - 4;
      if (ti >= 0 && ti < ntiles)
        write_tile_rows<T, kPreRow, 8>(t_xh + sel(ti), a.xh + kPitchBuf + ti * T, xh_stride, s0, a.n_streams, len_of(ti), lane);
    }
    __syncthreads();
  }
  if (valid && wave == 3) mhp.store(st);
  if (valid && wave == 1 && kDcHp) fe.store(a, NS, s);
}

// ---- The same pre-pass with the noise gate (dsp/gate.rs, realtime stage 1: dsp_loop.rs:1371-1435) after the front end.
// The gate is split so that no wave walks its whole per-sample chain (sqrt, log10, exp10 and the smoothing, ~100 dependent
// f64 instructions) as gate_lane_kernel does:
//   R1 (lane = stream, in the front-end wave)  rms_sq = c rms_sq + (1 - c) x^2                       (update_detector)
//   F1 (lane = TIME, four waves)               level = lin2db(sqrt(rms_sq)); bits level >= thr, level <= thr - 4, d > 24;
//                                              g36 = db_to_linear(-d), d = clamp((thr - level) 0.75, 0, 36)
//   R2 (lane = stream)                         hold / open / chatter / auto-relax state machine (track_gate_transition),
//                                              target 1, g36 or db_to_linear(-24) (= g36 whenever d <= 24: bit-identical
//                                              to clamping at 24 directly), attack / release smoothing, x gain
// Tiles are 32 samples (64 streams x 32 samples, rows of 65): the f64 tile R1 fills, F1 overwrites in place and R2 reads is
// in flight for three steps, the f32 tile for five (load, front end and gate work on it in place), which at 64-sample tiles
// would not fit the CU's LDS.  131 040 bytes: x[5] f32, g[3] f64, bits[3] u8, model input[2] + [2] f32.
// kSupp = false compiles the RNNoise roles out: scrub / clamp / DC / HP / gate over `n_samples`, result to `out`.  There
// `a.gate` = 0 runs the front end alone (the gate roles idle, the gate state is neither read nor written): the engine keeps
// the front end in this pass for the whole stream when the chain's route was chosen with it stripped.
constexpr int kGateTileT = 32;
constexpr int kGateTileElems = kGateTileT * kPreRow;
constexpr int kGateF1Waves = 4;
constexpr size_t kGateLds = sizeof(float) * 5 * kGateTileElems + sizeof(double) * 3 * kGateTileElems + 3 * kGateTileElems +
                            sizeof(float) * 4 * kGateTileElems;
static_assert(kGateLds <= 160 * 1024, "the gated pre-pass must fit one CU's LDS");
template <bool kSupp>
constexpr int gate_prepass_waves() { return kSupp ? 11 : 8; }
template <bool kSupp, bool kRaw>
__global__ __launch_bounds__(64 * gate_prepass_waves<kSupp>()) void supp_prefilter_gate_kernel(SuppArgs a) {
  extern __shared__ double gate_lds[];
  constexpr int T = kGateTileT;
  constexpr int kF1 = 2, kR2 = kF1 + kGateF1Waves, kSoft = kR2 + 1, kModelHp = kSoft + 1, kDryOut = kSupp ? kModelHp + 1 : kR2 + 1,
                kXhOut = kDryOut + 1;
  double *t_g = gate_lds;                                                                // [3]
  float *t_x = reinterpret_cast<float *>(t_g + 3 * kGateTileElems);                      // [5]
  float *t_sc = t_x + 5 * kGateTileElems, *t_xh = t_sc + 2 * kGateTileElems;             // [2], [2] (kSupp)
  uint8_t *t_b = reinterpret_cast<uint8_t *>(t_xh + 2 * kGateTileElems);                  // [3]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tl = lane & (T - 1), half = lane >> 5;  // lane = time roles: sample tl of rows half * 32 + r
  const int s0 = blockIdx.x * kPreGroup;
  const int s = s0 + lane;
  const bool valid = s < a.n_streams;
  const int sc = valid ? s : a.n_streams - 1;
  const int64_t NS = a.n_streams;
  const int64_t n = kSupp ? (int64_t)a.n_frames * kRnnFrame : a.n_samples;
  const int64_t col0 = kSupp ? a.frame0 * kRnnFrame : 0;
  const int64_t xh_stride = kPitchBuf + n;
  float *st = kSupp ? a.state + (int64_t)sc * SuppState::kCount : nullptr;
  const int64_t ntiles = (n + T - 1) / T;
  auto len_of = [&](int64_t ti) { return tile_len<T>(n, ti); };

  if (kSupp) copy_model_history<1>(a, s0, wave, gate_prepass_waves<kSupp>(), lane, xh_stride);

  int64_t *gs = a.gate_state;
  const bool gate_on = kSupp || a.gate != 0;
  ModelHp mhp;
  FrontEnd fe;
  GateDetector det;
  GateCore gc;
  if (wave == kModelHp && kSupp) mhp.load(st);
  if (wave == 1) {
    if (a.front_dc) fe.load(a, NS, sc);
    if (gate_on) det.load(gs, NS, sc);
  }
  if (wave == kR2 && gate_on) gc.load(gs, NS, sc);
  const double hb0 = a.hp_b0, hb1 = a.hp_b1, hb2 = a.hp_b2, ha1 = a.hp_a1, ha2 = a.hp_a2;
  const bool scrub = a.front_scrub != 0, clamp = a.front_clamp != 0, dc = a.front_dc != 0, hp_on = a.front_hp != 0;
  const double thr = a.gate_thr, thr_low = a.gate_thr - 4.0;
  // the two constant targets, evaluated by the same device routine as every other target
  const double g_open = db2lin(-0.0), g24 = db2lin(-24.0);
  constexpr int kLast = kSupp ? 6 : 4;  // the last role's lag in tiles

  for (int64_t it = 0; it < ntiles + kLast; ++it) {
    if (wave == 0) {  // ---- load tile `it` into x[it % 5]
      const int64_t ti = it;
      if (ti < ntiles) {
        const int len = len_of(ti);
        const int64_t col = col0 + ti * T + (tl < len ? tl : len - 1);
        float *tile = t_x + (ti % 5) * kGateTileElems;
#pragma unroll 1
        for (int r0 = half * 32; r0 < half * 32 + 32; r0 += 16) {  // (two batches of 16 loads in flight: the VGPR budget of 11 waves)
          float v[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) v[r] = a.in[(int64_t)row_of(a, s0, r0 + r) * a.in_stride + col];
#pragma unroll
          for (int r = 0; r < 16; ++r) tile[tl * kPreRow + r0 + r] = v[r];
        }
      }
    } else if (wave == 1) {  // ---- front end + R1 on tile it - 1, in place (lane = stream)
      const int64_t ti = it - 1;
      if (ti >= 0 && ti < ntiles) {
        const int len = len_of(ti);
        float *x = t_x + (ti % 5) * kGateTileElems;
        double *g = t_g + (ti % 3) * kGateTileElems;
#pragma unroll 4
        for (int t = 0; t < T; ++t) {
          if (t < len) {
            const float v = fe.step(x[t * kPreRow + lane], scrub, clamp, dc, hp_on, hb0, hb1, hb2, ha1, ha2);
            x[t * kPreRow + lane] = v;
            if (gate_on) g[t * kPreRow + lane] = det.step(v, a.gate_rms_c, a.gate_rms_omc);
          }
        }
      }
    } else if (wave >= kF1 && wave < kR2) {  // ---- F1 on tile it - 2 (lane = time): 16 streams per wave
      const int64_t ti = it - 2;
      if (gate_on && ti >= 0 && ti < ntiles && tl < len_of(ti)) {
        double *g = t_g + (ti % 3) * kGateTileElems;
        uint8_t *bits = t_b + (ti % 3) * kGateTileElems;
        const int rb = gate_f1_row<T>(wave - kF1, half);
#pragma unroll 2
        for (int j = 0; j < gate_f1_rows(T); ++j) {  // (a constant trip count whatever rb is)
          const int k = tl * kPreRow + rb + j;
          double level;
          bits[k] = (uint8_t)gate_level_part(g[k], thr, thr_low, level);
        }
      }
    } else if (wave == kR2) {  // ---- R2 on tile it - 3, in place (lane = stream)
      const int64_t ti = it - 3;
      if (gate_on && ti >= 0 && ti < ntiles) {
        const int len = len_of(ti);
        float *x = t_x + (ti % 5) * kGateTileElems;
        const double *g = t_g + (ti % 3) * kGateTileElems;
        const uint8_t *bits = t_b + (ti % 3) * kGateTileElems;
#pragma unroll 4
        for (int t = 0; t < T; ++t) {
          if (t < len) {
            const int k = t * kPreRow + lane;
            const int b = bits[k];
            gc.decide(b, a.gate_hold);
            // detector_gain_reduction_db: the range is the one in force BEFORE this sample's transition is tracked
            const double target = gc.open ? g_open : ((gc.relax > 0 && (b & 4)) ? g24 : g[k]);
            gc.track(gc.open, a.gate_vad_mode != 0, a.gate_window, a.gate_cooldown, a.gate_relax);
            gc.advance_timers();
            x[k] = gc.apply(x[k], target, a);
          }
        }
      }
    } else if (kSupp && wave == kSoft) {  // ---- model-input scaling of tile it - 4 (lane = time)
      const int64_t ti = it - 4;
      if (ti >= 0 && ti < ntiles)
        scale_tile_for_model<kRaw, T, kPreRow, 8>(t_x + (ti % 5) * kGateTileElems, t_sc + (ti & 1) * kGateTileElems, lane);
    } else if (kSupp && wave == kModelHp) {  // ---- the model's own high-pass on tile it - 5 (lane = stream)
      const int64_t ti = it - 5;
      if (ti >= 0 && ti < ntiles) {
        const int len = len_of(ti);
        const float *src = t_sc + (ti & 1) * kGateTileElems;
        float *dst = t_xh + (ti & 1) * kGateTileElems;
#pragma unroll 8
        for (int t = 0; t < T; ++t) {
          if (t < len) dst[t * kPreRow + lane] = mhp.step(src[t * kPreRow + lane]);
        }
      }
    } else if (wave == kDryOut) {  // ---- the gated signal of tile it - 4 to `out` (the suppressor's dry signal)
      const int64_t ti = it - 4;
      if (ti >= 0 && ti < ntiles)
        write_tile_rows<T, kPreRow, 8>(t_x + (ti % 5) * kGateTileElems, a.out + col0 + ti * T, a.stream_stride, s0, a.n_streams,
                                       len_of(ti), lane);
    } else if (kSupp && wave == kXhOut) {  // ---- the model input of tile it - 6
      const int64_t ti = it - 6;
      if (ti >= 0 && ti < ntiles)
        write_tile_rows<T, kPreRow, 8>(t_xh + (ti & 1) * kGateTileElems, a.xh + kPitchBuf + ti * T, xh_stride, s0, a.n_streams,
                                       len_of(ti), lane);
    }
    __syncthreads();
  }
  if (!valid) return;
  if (kSupp && wave == kModelHp) mhp.store(st);
  if (wave == 1) {
    if (a.front_dc) fe.store(a, NS, s);
    if (gate_on) det.store(gs, NS, s);
  }
  if (wave == kR2 && gate_on) gc.store(gs, NS, s);
}

// ============================================================================== the VAD-fused gate modes
// NoiseGate::process_block_inplace with a VadAutoGate::without_backend attached, modes VadAssisted / VadOnly
// (gate.rs:652-741).  Two passes per gate pass, on one stream:
//   vad_gate_control_kernel   per control block and stream: the controller (vad.rs:714-966).  It needs the RMS of the whole
//                             block of gate input before the block's first sample is gated, so it runs first, RECOMPUTES the
//                             front end from the raw input with a private copy of the front end's state (the state planes stay
//                             the per-sample pass's to advance; no second copy of the audio goes through memory) and leaves
//                             one decision row per (block, stream).
//   vad_gate_prepass_kernel   the gated pre-pass above with the fused per-sample path in its gate roles.
// vad_plane_init_kernel puts the state plane into VadAutoGate::without_backend / reset + NoiseGate::reset's fused fields.
__global__ void vad_plane_init_kernel(uint32_t *plane, int64_t n_streams, float closed_counter, int controller, int fused) {
  const int64_t total = (int64_t)kVadFields * n_streams;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int field = (int)(i / n_streams);
    const bool fused_field = field >= kVadSmoothed || field == kVadPrevProb;  // gate.rs:772-783
    if (fused_field ? !fused : !controller) continue;
    uint32_t v = 0;
    if (field == kVadFloor) v = __float_as_uint(-60.0f);
    if (field == kVadClosed) v = __float_as_uint(closed_counter);  // restarts "matured", vad.rs:650, 1022
    plane[i] = v;
  }
}
hipError_t launch_vad_plane_init(uint32_t *plane, int32_t n_streams, float closed_counter, bool controller, bool fused,
                                 hipStream_t stream) {
  hipLaunchKernelGGL(vad_plane_init_kernel, dim3(256), dim3(256), 0, stream, plane, (int64_t)n_streams, closed_counter,
                     controller ? 1 : 0, fused ? 1 : 0);
  return hipGetLastError();
}

// Two waves per 64 streams over 64-sample tiles, one barrier per tile: wave 0 loads tile i (lane = time, rows transposed
// into LDS), wave 1 (lane = stream) runs the front end on tile i-1, adds x^2 to the block's f32 sum in sample order and, at
// the end of every control block, steps the controller.  The histogram lives in LDS for the pass (61 x u16 per stream), the
// ring stays in memory (one read and one write per block).
constexpr int kCtlTile = 64 * kPreRow;
__global__ __launch_bounds__(128) void vad_gate_control_kernel(SuppArgs a, VadGateArgs v) {
  __shared__ float t_in[2 * kCtlTile];
  __shared__ uint16_t bins[kVadBinCount * kPreGroup];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s0 = blockIdx.x * kPreGroup;
  const int s = s0 + lane;
  const bool valid = s < a.n_streams;
  const int sc = valid ? s : a.n_streams - 1;
  const int64_t NS = a.n_streams;
  const bool supp = a.n_samples == 0;
  const int64_t n = supp ? (int64_t)a.n_frames * kRnnFrame : a.n_samples;
  const int64_t col0 = supp ? a.frame0 * kRnnFrame : 0;
  const int64_t ntiles = (n + 63) / 64;
  uint32_t *pl = v.plane;
  auto fld = [&](int f) -> uint32_t & { return pl[(int64_t)f * NS + sc]; };

  FrontEnd fe;  // a private copy, loaded and never stored: the per-sample pass advances the planes
  float sum = 0.0f;
  float floor_db = 0.0f, hold_timer = 0.0f, closed = 0.0f, prev_prob = 0.0f;
  int timer_running = 0, prev_open = 0, hist_len = 0, cursor = 0, in_block = 0;
  uint32_t last_flags = 0;
  int64_t blk = v.block0;
  if (wave == 1) {
    if (a.front_dc) fe.load(a, NS, sc);
    floor_db = __uint_as_float(fld(kVadFloor));
    hold_timer = __uint_as_float(fld(kVadHoldTimer));
    closed = __uint_as_float(fld(kVadClosed));
    prev_prob = __uint_as_float(fld(kVadPrevProb));
    timer_running = (int)fld(kVadTimerRunning);
    prev_open = (int)fld(kVadPrevOpen);
    hist_len = (int)fld(kVadHistLen);
    cursor = (int)fld(kVadCursor);
    last_flags = fld(kVadLastFlags);
    for (int b = 0; b < kVadBinCount; ++b) bins[b * kPreGroup + lane] = (uint16_t)fld(kVadBins + b);
  }
  const double hb0 = a.hp_b0, hb1 = a.hp_b1, hb2 = a.hp_b2, ha1 = a.hp_a1, ha2 = a.hp_a2;
  const bool scrub = a.front_scrub != 0, clamp = a.front_clamp != 0, dc = a.front_dc != 0, hp_on = a.front_hp != 0;
  auto bin_of = [](float db) {  // vad.rs:823-826
    const float raw = roundf((db - (-80.0f)) / 1.0f);
    return (int)fclamp(raw, 0.0f, (float)(kVadBinCount - 1));
  };

  for (int64_t it = 0; it < ntiles + 1; ++it) {
    if (wave == 0) {
      if (it < ntiles) {
        const int len = tile_len<64>(n, it);
        const int64_t col = col0 + it * 64 + (lane < len ? lane : len - 1);
        float *tile = t_in + (it & 1) * kCtlTile;
#pragma unroll 1
        for (int r0 = 0; r0 < kPreGroup; r0 += 16) {
          float x[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) x[r] = a.in[(int64_t)row_of(a, s0, r0 + r) * a.in_stride + col];
#pragma unroll
          for (int r = 0; r < 16; ++r) tile[lane * kPreRow + r0 + r] = x[r];
        }
      }
    } else if (it >= 1) {
      const int64_t ti = it - 1;
      const int len = tile_len<64>(n, ti);
      const float *tile = t_in + (ti & 1) * kCtlTile;
      for (int t = 0; t < len; ++t) {
        const float x = fe.step(tile[t * kPreRow + lane], scrub, clamp, dc, hp_on, hb0, hb1, hb2, ha1, ha2);
        sum += x * x;  // compute_rms_db, vad.rs:1086-1099: f32, in sample order
        ++in_block;
        if (in_block == v.block || ti * 64 + t + 1 == n) {
          // ---- process_with_external_probability, vad.rs:714-726
          const int64_t ei = v.ev_stride ? blk * v.ev_stride + sc : blk;
          const bool avail = v.prob && v.avail[ei] != 0;
          const float prob = avail ? fclamp(v.prob[ei], 0.0f, 1.0f) : 0.0f;
          const float rms = sqrtf(sum / (float)in_block);
          const float rms_db = rms < 1e-6f ? -120.0f : 20.0f * log10f(rms);
          // ---- update_noise_floor_estimate, vad.rs:728-761 over push_noise_floor_sample :763-780, percentile :786-802
          if (v.auto_threshold && prob < 0.3f && rms_db > -100.0f) {
            const int bin = bin_of(rms_db);
            if (hist_len < kVadHistory) {
              if (valid) fld(kVadHist + hist_len) = __float_as_uint(rms_db);
              hist_len += 1;
              bins[bin * kPreGroup + lane] += 1;
            } else {
              const int old_bin = bin_of(__uint_as_float(fld(kVadHist + cursor)));
              uint16_t &ob = bins[old_bin * kPreGroup + lane];
              if (ob > 0) ob -= 1;
              if (valid) fld(kVadHist + cursor) = __float_as_uint(rms_db);
              bins[bin * kPreGroup + lane] += 1;
              cursor = (cursor + 1) % kVadHistory;
            }
            int target = (int)floorf((float)hist_len * 0.20f);
            target = target < hist_len - 1 ? target : hist_len - 1;
            int cumulative = 0, found = -1;
            for (int b = 0; b < kVadBinCount; ++b) {
              cumulative += bins[b * kPreGroup + lane];
              if (found < 0 && cumulative > target) found = b;
            }
            const float candidate = found >= 0 ? -80.0f + (float)found * 1.0f : floor_db;
            const float delta = candidate - floor_db;
            floor_db += delta > 0.0f ? fminf(delta, 0.5f) : fmaxf(delta, -0.1f);
            floor_db = fclamp(floor_db, -80.0f, -20.0f);
          }
          // ---- level_above_threshold, vad.rs:912-923; the mode's raw decision, :849-880
          const float threshold = v.auto_threshold ? fclamp(floor_db + v.margin_db, -80.0f, -10.0f)
                                                   : fclamp(v.manual_threshold_db, -80.0f, -10.0f);
          const bool level = rms_db >= threshold;
          const bool speech = prob > v.vad_threshold;
          const bool gate_open = v.mode == 1 ? (level || speech) : speech;
          // ---- apply_hold_time, vad.rs:925-966
          const bool rising = gate_open && !prev_open;
          const bool debounced = (rising && !(closed >= v.debounce_samples)) ? false : gate_open;
          if (debounced) {
            hold_timer = v.hold_samples;
            timer_running = 1;
            closed = 0.0f;
          } else {
            closed += (float)in_block;
          }
          if (timer_running) {
            hold_timer -= (float)in_block;
            if (hold_timer <= 0.0f) {
              hold_timer = 0.0f;
              timer_running = 0;
            }
          }
          prev_open = debounced ? 1 : 0;
          last_flags = ((debounced || timer_running) ? kVadDecHeld : 0u) | (avail ? kVadDecAvail : 0u);
          if (valid) {
            uint32_t *row = v.dec + blk * kVadDecWords * NS + s;
            row[kVadDecProb * NS] = __float_as_uint(prob);
            row[kVadDecDelta * NS] = __float_as_uint(prob - prev_prob);  // gate.rs:669
            row[kVadDecFlags * NS] = last_flags;
            row[kVadDecFloor * NS] = __float_as_uint(floor_db);
          }
          prev_prob = prob;  // gate.rs:736
          sum = 0.0f;
          in_block = 0;
          ++blk;
        }
      }
    }
    __syncthreads();
  }
  if (wave == 1 && valid) {
    fld(kVadFloor) = __float_as_uint(floor_db);
    fld(kVadHoldTimer) = __float_as_uint(hold_timer);
    fld(kVadClosed) = __float_as_uint(closed);
    fld(kVadPrevProb) = __float_as_uint(prev_prob);
    fld(kVadTimerRunning) = (uint32_t)timer_running;
    fld(kVadPrevOpen) = (uint32_t)prev_open;
    fld(kVadHistLen) = (uint32_t)hist_len;
    fld(kVadCursor) = (uint32_t)cursor;
    fld(kVadLastFlags) = last_flags;
    for (int b = 0; b < kVadBinCount; ++b) fld(kVadBins + b) = bins[b * kPreGroup + lane];
  }
}

// The per-sample pass.  Roles as in supp_prefilter_gate_kernel; what the fused path adds to each:
//   R1 (lane = stream)  vad_smoothed_probability: one pole towards the block's probability, f64, stored as f32 per sample
//                       (gate.rs:700-705), and the block's held-open / availability bits beside each sample
//   F1 (lane = TIME)    level_open_score (gate.rs:307-313, f32), the smoothstep posterior reduction (gate.rs:485-527) and the
//                       gain it alone would ask for under either range: p36 = db_to_linear(-36 c s), p24 = db_to_linear(-24 c s)
//   R2 (lane = stream)  fused score and its hysteresis (gate.rs:315-366), the five-state machine (:374-483), then
//                       target = force_close ? db_to_linear(-range) : min(level gain, posterior gain)
//                       -- db_to_linear(-max(a, b)) = min(db_to_linear(-a), db_to_linear(-b)) for a monotone db_to_linear, so R2
//                       only selects, as it does with g36 and the 24 dB constant -- chatter tracking on the FUSED open state
//                       (gate.rs:732-733), smoothing, x gain.
// Tiles are 16 samples here (64 streams x 16, rows of 65): F1 hands R2 three f64 values per sample instead of one, and at 32
// samples that would not fit the CU's LDS beside the suppressor's model-input tiles.  115 440 bytes: g[3] p36[2] p24[2] f64,
// x[5] smoothed[2] score[2] model input[2] + [2] f32, bits[3] u8.  A pass starts on a control-block boundary (the call, or
// a suppressor window of whole control blocks), so R1 and R2 count samples to find the next decision row.
constexpr int kVgT = 16;
constexpr int kVgElems = kVgT * kPreRow;
constexpr size_t kVadGateLds = sizeof(double) * 7 * kVgElems + sizeof(float) * 13 * kVgElems + 3 * kVgElems;
static_assert(kVadGateLds <= 160 * 1024, "the VAD-fused pre-pass must fit one CU's LDS");
template <bool kSupp, bool kRaw>
__global__ __launch_bounds__(64 * gate_prepass_waves<kSupp>()) void vad_gate_prepass_kernel(SuppArgs a, VadGateArgs v) {
  extern __shared__ double vg_lds[];
  constexpr int T = kVgT, kRows = T;  // lane = time roles: sample tl of rows grp * T + r, r < T (64 / T groups of T rows)
  constexpr int kF1 = 2, kR2 = kF1 + kGateF1Waves, kSoft = kR2 + 1, kModelHp = kSoft + 1, kDryOut = kSupp ? kModelHp + 1 : kR2 + 1,
                kXhOut = kDryOut + 1;
  double *t_g = vg_lds;                                                     // [3]
  double *t_p36 = t_g + 3 * kVgElems, *t_p24 = t_p36 + 2 * kVgElems;         // [2], [2]
  float *t_x = reinterpret_cast<float *>(t_p24 + 2 * kVgElems);             // [5]
  float *t_sm = t_x + 5 * kVgElems, *t_ls = t_sm + 2 * kVgElems;            // [2], [2]
  float *t_sc = t_ls + 2 * kVgElems, *t_xh = t_sc + 2 * kVgElems;           // [2], [2] (kSupp)
  uint8_t *t_b = reinterpret_cast<uint8_t *>(t_xh + 2 * kVgElems);          // [3]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tl = lane & (T - 1), grp = lane / T;
  const int s0 = blockIdx.x * kPreGroup;
  const int s = s0 + lane;
  const bool valid = s < a.n_streams;
  const int sc = valid ? s : a.n_streams - 1;
  const int64_t NS = a.n_streams;
  const int64_t n = kSupp ? (int64_t)a.n_frames * kRnnFrame : a.n_samples;
  const int64_t col0 = kSupp ? a.frame0 * kRnnFrame : 0;
  const int64_t xh_stride = kPitchBuf + n;
  float *st = kSupp ? a.state + (int64_t)sc * SuppState::kCount : nullptr;
  const int64_t ntiles = (n + T - 1) / T;
  auto len_of = [&](int64_t ti) { return tile_len<T>(n, ti); };

  if (kSupp) copy_model_history<1>(a, s0, wave, gate_prepass_waves<kSupp>(), lane, xh_stride);

  int64_t *gs = a.gate_state;
  uint32_t *pl = v.plane;
  ModelHp mhp;
  FrontEnd fe;
  GateDetector det;
  GateCore gc;
  bool fused_open = false;
  int gstate = 0, in_block = 0;
  int64_t blk = v.block0;
  float sm = 0.0f, fused_score = 0.0f, prob = 0.0f, pdelta = 0.0f;
  uint32_t dflags = 0;
  if (wave == kModelHp && kSupp) mhp.load(st);
  if (wave == 1) {
    if (a.front_dc) fe.load(a, NS, sc);
    det.load(gs, NS, sc);
    sm = __uint_as_float(pl[(int64_t)kVadSmoothed * NS + sc]);
  }
  if (wave == kR2) {
    gc.load(gs, NS, sc);
    fused_score = __uint_as_float(pl[(int64_t)kVadFusedScore * NS + sc]);
    fused_open = pl[(int64_t)kVadFusedOpen * NS + sc] != 0;
    gstate = (int)pl[(int64_t)kVadGateState * NS + sc];
  }
  auto load_decision = [&]() {  // this wave's lane = its stream: rows are read coalesced
    const uint32_t *row = v.dec + blk * kVadDecWords * NS + sc;
    prob = __uint_as_float(row[kVadDecProb * NS]);
    pdelta = __uint_as_float(row[kVadDecDelta * NS]);
    dflags = row[kVadDecFlags * NS];
  };
  const double hb0 = a.hp_b0, hb1 = a.hp_b1, hb2 = a.hp_b2, ha1 = a.hp_a1, ha2 = a.hp_a2;
  const bool scrub = a.front_scrub != 0, clamp = a.front_clamp != 0, dc = a.front_dc != 0, hp_on = a.front_hp != 0;
  const double thr = a.gate_thr, thr_low = a.gate_thr - 4.0, thr_span = thr - thr_low;
  const double g_open = db2lin(-0.0), g24 = db2lin(-24.0), g36c = db2lin(-36.0);
  // update_probabilistic_gate_state's and probability_speech_confidence's thresholds (gate.rs:392-393, 488-491), f32
  // (f32, evaluated once on the host: this target has no scalar float unit, and as vector values they would cost every wave
  // of the workgroup six registers)
  const float open_thr = v.open_thr, close_norm = v.close_norm, close_relax = v.close_relax;
  const float conf_close = v.conf_close, conf_span = v.conf_span, tail_thr = v.tail_thr;
  const double post_scale = v.mode == 1 ? 0.30 : 0.45;             // gate.rs:521-525
  const bool assisted = v.mode == 1;
  constexpr int kLast = kSupp ? 6 : 4;  // the last role's lag in tiles

  for (int64_t it = 0; it < ntiles + kLast; ++it) {
    if (wave == 0) {  // ---- load tile `it` into x[it % 5]
      const int64_t ti = it;
      if (ti < ntiles) {
        const int len = len_of(ti);
        const int64_t col = col0 + ti * T + (tl < len ? tl : len - 1);
        float *tile = t_x + (ti % 5) * kVgElems;
#pragma unroll 1
        for (int r0 = grp * kRows; r0 < grp * kRows + kRows; r0 += 8) {  // (two batches of 8 loads in flight: the VGPR budget of 11 waves)
          float x[8];
#pragma unroll
          for (int r = 0; r < 8; ++r) x[r] = a.in[(int64_t)row_of(a, s0, r0 + r) * a.in_stride + col];
#pragma unroll
          for (int r = 0; r < 8; ++r) tile[tl * kPreRow + r0 + r] = x[r];
        }
      }
    } else if (wave == 1) {  // ---- front end + R1 on tile it - 1, in place (lane = stream)
      const int64_t ti = it - 1;
      if (ti >= 0 && ti < ntiles) {
        const int len = len_of(ti);
        float *x = t_x + (ti % 5) * kVgElems;
        double *g = t_g + (ti % 3) * kVgElems;
        float *smo = t_sm + (ti & 1) * kVgElems;
        uint8_t *bits = t_b + (ti % 3) * kVgElems;
#pragma unroll 1
        for (int t = 0; t < T; ++t) {
          if (t < len) {
            if (in_block == 0) load_decision();
            if (++in_block == v.block) {
              in_block = 0;
              ++blk;
            }
            const float xv = fe.step(x[t * kPreRow + lane], scrub, clamp, dc, hp_on, hb0, hb1, hb2, ha1, ha2);
            x[t * kPreRow + lane] = xv;
            g[t * kPreRow + lane] = det.step(xv, a.gate_rms_c, a.gate_rms_omc);
            sm = (float)dclamp(v.smooth_c * (double)sm + v.smooth_omc * (double)prob, 0.0, 1.0);  // gate.rs:700-705
            smo[t * kPreRow + lane] = sm;
            bits[t * kPreRow + lane] = (uint8_t)(((dflags & kVadDecHeld) ? 8 : 0) | ((dflags & kVadDecAvail) ? 16 : 0));
          }
        }
      }
    } else if (wave >= kF1 && wave < kR2) {  // ---- F1 on tile it - 2 (lane = time): 16 streams per wave
      const int64_t ti = it - 2;
      if (ti >= 0 && ti < ntiles && tl < len_of(ti)) {
        double *g = t_g + (ti % 3) * kVgElems;
        double *p36 = t_p36 + (ti & 1) * kVgElems, *p24 = t_p24 + (ti & 1) * kVgElems;
        const float *smo = t_sm + (ti & 1) * kVgElems;
        float *ls = t_ls + (ti & 1) * kVgElems;
        uint8_t *bits = t_b + (ti % 3) * kVgElems;
        const int rb = gate_f1_row<T>(wave - kF1, grp);
#pragma unroll 1
        for (int j = 0; j < gate_f1_rows(T); ++j) {  // (a constant trip count whatever rb is)
          const int k = tl * kPreRow + rb + j;
          double level;
          const int level_bits = gate_level_part(g[k], thr, thr_low, level);
          ls[k] = (float)dclamp((level - thr_low) / thr_span, 0.0, 1.0);        // gate.rs:307-313
          const int fl = bits[k];
          double q36 = g_open, q24 = g_open;
          if (fl & 16) {  // continuous_vad_gain_reduction_db, gate.rs:498-527
            const float p = smo[k];
            const double nrm = (double)fclamp((p - conf_close) / conf_span, 0.0f, 1.0f);
            double closure = 1.0 - nrm * nrm * (3.0 - 2.0 * nrm);
            if ((fl & 8) && p >= tail_thr) closure = fmin(closure, 0.80);
            q36 = db2lin(-(36.0 * closure * post_scale));
            q24 = db2lin(-(24.0 * closure * post_scale));
          }
          p36[k] = q36;
          p24[k] = q24;
          bits[k] = (uint8_t)(fl | level_bits);
        }
      }
    } else if (wave == kR2) {  // ---- R2 on tile it - 3, in place (lane = stream)
      const int64_t ti = it - 3;
      if (ti >= 0 && ti < ntiles) {
        const int len = len_of(ti);
        float *x = t_x + (ti % 5) * kVgElems;
        const double *g = t_g + (ti % 3) * kVgElems;
        const double *p36 = t_p36 + (ti & 1) * kVgElems, *p24 = t_p24 + (ti & 1) * kVgElems;
        const float *ls = t_ls + (ti & 1) * kVgElems;
        const uint8_t *bits = t_b + (ti % 3) * kVgElems;
#pragma unroll 1
        for (int t = 0; t < T; ++t) {
          if (t < len) {
            if (in_block == 0) load_decision();
            if (++in_block == v.block) {
              in_block = 0;
              ++blk;
            }
            const int k = t * kPreRow + lane;
            const int b = bits[k];
            gc.decide(b, a.gate_hold);
            const bool held = (b & 8) != 0, avail = (b & 16) != 0;
            const float level_score = ls[k];
            // update_fused_gate_score, gate.rs:315-366 (the probability is clamped where the decision row is written)
            const float recent = (fused_open || gc.gain > 0.35) ? 1.0f : 0.0f;
            if (assisted) {
              if (avail) {
                const float blended = fclamp(0.55f * level_score + 0.45f * prob + 0.10f * recent, 0.0f, 1.0f);
                fused_score = fmaxf(fmaxf(level_score, prob), blended);
              } else {
                fused_score = 0.85f * level_score + 0.15f * recent;
              }
            } else {
              fused_score = avail ? (held ? fmaxf(prob, 0.55f) : prob) : (held ? 0.55f : 0.0f);
            }
            if (fused_score >= 0.55f) {
              fused_open = true;
            } else if (fused_score <= 0.35f) {
              fused_open = false;
            }
            // update_probabilistic_gate_state, gate.rs:374-483
            const bool auto_relax = gc.relax > 0;
            const float close_thr = auto_relax ? close_relax : close_norm;
            const bool vad_open = avail && (prob >= open_thr || (pdelta >= 0.08f && prob >= close_thr));
            const bool vad_uncertain = avail && prob >= close_thr;
            const bool level_open = gc.open || level_score >= 0.55f;
            const bool level_uncertain = level_score >= 0.22f || gc.gain > 0.12;
            const bool carry = !avail || vad_uncertain || gc.gain > 0.20;
            bool strong_open, sustain;
            if (assisted) {
              strong_open = (level_open && carry) || (fused_open && carry) || (held && carry) || vad_open;
              sustain = strong_open || vad_uncertain || level_uncertain || (auto_relax && level_score > 0.08f);
            } else {
              strong_open = held || vad_open;
              sustain = strong_open || vad_uncertain || (auto_relax && gc.gain > 0.12);
            }
            const bool releasing_sustain = sustain || (gc.gain > 0.20 && (vad_uncertain || auto_relax));
            const int fall = sustain ? 3 : (releasing_sustain ? 4 : 0);
            if (gstate == 0) {
              gstate = strong_open ? 1 : 0;
            } else if (gstate == 1) {
              gstate = strong_open ? 2 : (sustain ? 3 : 0);
            } else if (gstate == 2) {
              gstate = strong_open ? 2 : fall;
            } else {
              gstate = strong_open ? 1 : fall;
            }
            const bool prob_open = gstate != 0;  // force_close = !prob_open, effective_open = prob_open (gate.rs:722-733)
            // compute_vad_target_gr_db, gate.rs:529-553, with the range in force BEFORE this sample's transition is tracked
            const double level_gain = gc.open ? g_open : ((auto_relax && (b & 4)) ? g24 : g[k]);
            const double target = prob_open ? fmin(level_gain, auto_relax ? p24[k] : p36[k]) : (auto_relax ? g24 : g36c);
            gc.track(prob_open, true, a.gate_window, a.gate_cooldown, a.gate_relax);  // chatter on the FUSED state, gate.rs:732-733
            gc.advance_timers();
            x[k] = gc.apply(x[k], target, a);
          }
        }
      }
    } else if (kSupp && wave == kSoft) {  // ---- model-input scaling of tile it - 4 (lane = time)
      const int64_t ti = it - 4;
      if (ti >= 0 && ti < ntiles)
        scale_tile_for_model<kRaw, T, kPreRow, 4>(t_x + (ti % 5) * kVgElems, t_sc + (ti & 1) * kVgElems, lane);
    } else if (kSupp && wave == kModelHp) {  // ---- the model's own high-pass on tile it - 5 (lane = stream)
      const int64_t ti = it - 5;
      if (ti >= 0 && ti < ntiles) {
        const int len = len_of(ti);
        const float *src = t_sc + (ti & 1) * kVgElems;
        float *dst = t_xh + (ti & 1) * kVgElems;
#pragma unroll 8
        for (int t = 0; t < T; ++t) {
          if (t < len) dst[t * kPreRow + lane] = mhp.step(src[t * kPreRow + lane]);
        }
      }
    } else if (wave == kDryOut) {  // ---- the gated signal of tile it - 4 to `out` (the suppressor's dry signal)
      const int64_t ti = it - 4;
      if (ti >= 0 && ti < ntiles)
        write_tile_rows<T, kPreRow, 4>(t_x + (ti % 5) * kVgElems, a.out + col0 + ti * T, a.stream_stride, s0, a.n_streams, len_of(ti),
                                       lane);
    } else if (kSupp && wave == kXhOut) {  // ---- the model input of tile it - 6
      const int64_t ti = it - 6;
      if (ti >= 0 && ti < ntiles)
        write_tile_rows<T, kPreRow, 4>(t_xh + (ti & 1) * kVgElems, a.xh + kPitchBuf + ti * T, xh_stride, s0, a.n_streams, len_of(ti),
                                       lane);
    }
    __syncthreads();
  }
  if (!valid) return;
  if (kSupp && wave == kModelHp) mhp.store(st);
  if (wave == 1) {
    if (a.front_dc) fe.store(a, NS, s);
    det.store(gs, NS, s);
    pl[(int64_t)kVadSmoothed * NS + s] = __float_as_uint(sm);
  }
  if (wave == kR2) {
    gc.store(gs, NS, s);
    pl[(int64_t)kVadFusedScore * NS + s] = __float_as_uint(fused_score);
    pl[(int64_t)kVadFusedOpen * NS + s] = fused_open ? 1u : 0u;
    pl[(int64_t)kVadGateState * NS + s] = (uint32_t)gstate;
  }
}

// ============================================================================== launch
// The sample-serial pre-pass of a window (independent of the other kernels: it may run a window ahead).
template <bool kClamp, bool kDcHp, bool kRaw>
static hipError_t launch_prefilter_variant(const SuppArgs &a, hipStream_t stream) {
  constexpr size_t lds = sizeof(float) * 2 * kPreRing * kPreTile;  // 49 920 bytes at 32-sample tiles
  static_assert(lds <= 65536 + sizeof(float) * 2 * kPreRing * kPreT || kPreT > 32, "the pre-pass leaves room for transform workgroups beside it");
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(supp_prefilter_kernel<kClamp, kDcHp, kRaw>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return err;
    attr_set = true;
  }
  const dim3 grid((a.n_streams + kPreGroup - 1) / kPreGroup), block(64 * kPreWaves);
  hipLaunchKernelGGL((supp_prefilter_kernel<kClamp, kDcHp, kRaw>), grid, block, lds, stream, a);
  return hipGetLastError();
}
template <bool kSupp, bool kRaw>
static hipError_t launch_prefilter_gate_variant(const SuppArgs &a, hipStream_t stream) {
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(supp_prefilter_gate_kernel<kSupp, kRaw>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)kGateLds);
    if (err != hipSuccess) return err;
    attr_set = true;
  }
  const dim3 grid((a.n_streams + kPreGroup - 1) / kPreGroup), block(64 * gate_prepass_waves<kSupp>());
  hipLaunchKernelGGL((supp_prefilter_gate_kernel<kSupp, kRaw>), grid, block, kGateLds, stream, a);
  return hipGetLastError();
}
// The VAD-fused gate pass: the control pass, then the per-sample pass (kSupp: a.n_samples == 0, a window of whole frames).
template <bool kSupp, bool kRaw>
static hipError_t launch_vad_gate_variant(const SuppArgs &a, const VadGateArgs &v, hipStream_t stream) {
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(vad_gate_prepass_kernel<kSupp, kRaw>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)kVadGateLds);
    if (err != hipSuccess) return err;
    attr_set = true;
  }
  const dim3 grid((a.n_streams + kPreGroup - 1) / kPreGroup);
  hipLaunchKernelGGL(vad_gate_control_kernel, grid, dim3(128), 0, stream, a, v);
  hipLaunchKernelGGL((vad_gate_prepass_kernel<kSupp, kRaw>), grid, dim3(64 * gate_prepass_waves<kSupp>()), kVadGateLds, stream, a, v);
  return hipGetLastError();
}
hipError_t launch_vad_gate_pass(const SuppArgs &a, const VadGateArgs &v, hipStream_t stream) {
  if (a.n_samples > 0) return launch_vad_gate_variant<false, false>(a, v, stream);
  return a.raw_protocol ? launch_vad_gate_variant<true, true>(a, v, stream) : launch_vad_gate_variant<true, false>(a, v, stream);
}
// the gated front end without the suppressor: `in` -> `out` over a.n_samples
hipError_t launch_gate_prepass(const SuppArgs &a, hipStream_t stream) { return launch_prefilter_gate_variant<false, false>(a, stream); }
hipError_t launch_suppressor_prefilter(const SuppArgs &a, hipStream_t stream) {
  if (a.gate) return a.raw_protocol ? launch_prefilter_gate_variant<true, true>(a, stream) : launch_prefilter_gate_variant<true, false>(a, stream);
  const int sel = (a.front_clamp ? 4 : 0) | (a.front_dc ? 2 : 0) | (a.raw_protocol ? 1 : 0);
  switch (sel) {
    case 0: return launch_prefilter_variant<false, false, false>(a, stream);
    case 1: return launch_prefilter_variant<false, false, true>(a, stream);
    case 2: return launch_prefilter_variant<false, true, false>(a, stream);
    case 3: return launch_prefilter_variant<false, true, true>(a, stream);
    case 4: return launch_prefilter_variant<true, false, false>(a, stream);
    case 5: return launch_prefilter_variant<true, false, true>(a, stream);
    case 6: return launch_prefilter_variant<true, true, false>(a, stream);
    default: return launch_prefilter_variant<true, true, true>(a, stream);
  }
}

}  // namespace af
