// af_suppressor_host.hpp -- host side of the RNNoise suppressor stage: weights, tables, workspace.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "af_hip_resources.hpp"
#include "af_suppressor.h"
#include "af_switches.hpp"

namespace af {

hipError_t launch_suppressor_analysis(const SuppArgs &a, const SuppTables &tb, hipStream_t stream);
// its three launches, in order (launch_suppressor_analysis calls exactly these)
hipError_t launch_suppressor_spectrum(const SuppArgs &a, const SuppTables &tb, hipStream_t stream);
hipError_t launch_suppressor_pitch_search(const SuppArgs &a, const SuppTables &tb, hipStream_t stream);
hipError_t launch_suppressor_pitch_tracker(const SuppArgs &a, const SuppTables &tb, hipStream_t stream);
hipError_t launch_suppressor_synthesis(const SuppArgs &a, const SuppTables &tb, const RnnDeviceWeights &w, hipStream_t stream,
                                       hipEvent_t after_network, hipStream_t finish_stream);
hipError_t launch_suppressor_prefilter(const SuppArgs &a, hipStream_t stream);
hipError_t launch_gate_prepass(const SuppArgs &a, hipStream_t stream);  // the gated front end without the suppressor
// the VAD-fused gate modes: control pass + per-sample pass (a.n_samples > 0: without the suppressor, else one window of frames)
hipError_t launch_vad_gate_pass(const SuppArgs &a, const VadGateArgs &v, hipStream_t stream);
hipError_t launch_vad_plane_init(uint32_t *plane, int32_t n_streams, float closed_counter, bool controller, bool fused, hipStream_t stream);
hipError_t launch_scale_probe(const float *in, float *out, int64_t n, hipStream_t stream);

// int8 network weights in the layout of the public RNNoise model (dense: [in][out]; GRU: [in][3*units],
// gate order z | r | h).  The trained weights of nnnoiseless 0.5.2 are embedded in that crate and are not
// available offline, so engines start from seeded synthetic weights; a real blob (the fifteen arrays
// below, concatenated in declaration order) can be loaded with af_suppressor_load_weights().
struct RnnWeightsI8 {
  int8_t input_dense_w[42 * 24], input_dense_b[24];
  int8_t vad_gru_w[24 * 72], vad_gru_u[24 * 72], vad_gru_b[72];
  int8_t vad_out_w[24 * 1], vad_out_b[1];
  int8_t noise_gru_w[90 * 144], noise_gru_u[48 * 144], noise_gru_b[144];
  int8_t denoise_gru_w[114 * 288], denoise_gru_u[96 * 288], denoise_gru_b[288];
  int8_t denoise_out_w[96 * 22], denoise_out_b[22];
};
static_assert(sizeof(RnnWeightsI8) == 42 * 24 + 24 + 2 * 24 * 72 + 72 + 24 + 1 + 90 * 144 + 48 * 144 + 144 +
                                          114 * 288 + 96 * 288 + 288 + 96 * 22 + 22,
              "weight blob layout");

inline uint64_t splitmix(uint64_t *s) {
  uint64_t z = (*s += 0x9E3779B97F4A7C15ULL);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}
inline void fill_i8(int8_t *dst, size_t n, uint64_t *s, int amp) {
  for (size_t i = 0; i < n; ++i) {
    const int a = (int)(splitmix(s) % (uint64_t)(2 * amp + 1)) - amp;
    const int b = (int)(splitmix(s) % (uint64_t)(2 * amp + 1)) - amp;
    dst[i] = (int8_t)((a + b) / 2);
  }
}
inline void synthetic_weights(RnnWeightsI8 &w, uint64_t seed) {
  uint64_t s = seed;
  fill_i8(w.input_dense_w, sizeof w.input_dense_w, &s, 48);
  fill_i8(w.input_dense_b, sizeof w.input_dense_b, &s, 20);
  fill_i8(w.vad_gru_w, sizeof w.vad_gru_w, &s, 40);
  fill_i8(w.vad_gru_u, sizeof w.vad_gru_u, &s, 40);
  fill_i8(w.vad_gru_b, sizeof w.vad_gru_b, &s, 20);
  fill_i8(w.vad_out_w, sizeof w.vad_out_w, &s, 60);
  fill_i8(w.vad_out_b, sizeof w.vad_out_b, &s, 20);
  fill_i8(w.noise_gru_w, sizeof w.noise_gru_w, &s, 30);
  fill_i8(w.noise_gru_u, sizeof w.noise_gru_u, &s, 30);
  fill_i8(w.noise_gru_b, sizeof w.noise_gru_b, &s, 20);
  fill_i8(w.denoise_gru_w, sizeof w.denoise_gru_w, &s, 24);
  fill_i8(w.denoise_gru_u, sizeof w.denoise_gru_u, &s, 24);
  fill_i8(w.denoise_gru_b, sizeof w.denoise_gru_b, &s, 20);
  fill_i8(w.denoise_out_w, sizeof w.denoise_out_w, &s, 60);
  fill_i8(w.denoise_out_b, sizeof w.denoise_out_b, &s, 40);
}

// What upload() sends to the device, built on the host alone (build_suppressor_blob makes no HIP call): the f32 blob -- each
// of the eleven matrices of kRnnMatrixDims, padded to the matrix-core tiles ([k_pad][n_pad], a GRU's recurrent rows behind its
// input rows, padding zero), followed by its bias, then the tables -- the same matrices as int8 in the network kernel's
// operand order (w4_matrix_offset, af_suppressor.h), and where each part of the blob starts, in floats.
struct SuppressorBlob {
  std::vector<float> f32;
  std::vector<uint32_t> w4;
  size_t matrix[11], bias[11];  // in the order of kRnnMatrixDims: dense, vad z r h, noise z r h, denoise z r h, out
  size_t tansig, half_window, dct, twiddle, frac, band_of_bin;
};

// matrix `i`: columns [gate n, gate n + n) of `w` (and of the recurrent `u`, if the layer has one), whose rows hold `gates` x n
inline void append_matrix(SuppressorBlob &out, int i, const int8_t *w, const int8_t *u, const int8_t *b, int gate, int gates) {
  const RnnLayerDims d = kRnnMatrixDims[i];
  const int stride = gates * d.n, col0 = gate * d.n;
  std::vector<float> &dst = out.f32;
  const size_t off_w = out.matrix[i] = dst.size();
  dst.resize(dst.size() + (size_t)d.k_pad * d.n_pad, 0.0f);
  for (int k = 0; k < d.k_in; ++k)
    for (int n = 0; n < d.n; ++n) dst[off_w + (size_t)k * d.n_pad + n] = (float)w[k * stride + col0 + n];
  for (int k = 0; k < d.k_rec; ++k)
    for (int n = 0; n < d.n; ++n) dst[off_w + (size_t)(d.k_in + k) * d.n_pad + n] = (float)u[k * stride + col0 + n];
  const size_t off_b = out.bias[i] = dst.size();
  dst.resize(dst.size() + d.n_pad, 0.0f);
  for (int n = 0; n < d.n; ++n) dst[off_b + n] = (float)b[col0 + n];
}

inline SuppressorBlob build_suppressor_blob(const RnnWeightsI8 &weights) {
  SuppressorBlob out;
  std::vector<float> &blob = out.f32;
  append_matrix(out, 0, weights.input_dense_w, nullptr, weights.input_dense_b, 0, 1);
  for (int g = 0; g < 3; ++g) append_matrix(out, 1 + g, weights.vad_gru_w, weights.vad_gru_u, weights.vad_gru_b, g, 3);
  for (int g = 0; g < 3; ++g) append_matrix(out, 4 + g, weights.noise_gru_w, weights.noise_gru_u, weights.noise_gru_b, g, 3);
  for (int g = 0; g < 3; ++g) append_matrix(out, 7 + g, weights.denoise_gru_w, weights.denoise_gru_u, weights.denoise_gru_b, g, 3);
  append_matrix(out, 10, weights.denoise_out_w, nullptr, weights.denoise_out_b, 0, 1);
  const double pi = 3.14159265358979323846;
  out.tansig = blob.size();
  for (int i = 0; i <= 200; ++i) blob.push_back((float)std::tanh(0.04 * i));
  while (blob.size() % 4) blob.push_back(0.0f);
  out.half_window = blob.size();
  for (int i = 0; i < kRnnFrame; ++i) {
    const double sn = std::sin(.5 * pi * (i + .5) / kRnnFrame);
    blob.push_back((float)std::sin(.5 * pi * sn * sn));
  }
  out.dct = blob.size();
  for (int i = 0; i < kRnnBands; ++i)
    for (int j = 0; j < kRnnBands; ++j) {
      double v = std::cos((i + .5) * j * pi / kRnnBands);
      if (j == 0) v *= std::sqrt(.5);
      blob.push_back((float)v);
    }
  while (blob.size() % 4) blob.push_back(0.0f);
  out.twiddle = blob.size();
  for (int i = 0; i < kRnnWindow; ++i) {
    blob.push_back((float)std::cos(-2.0 * pi * i / kRnnWindow));
    blob.push_back((float)std::sin(-2.0 * pi * i / kRnnWindow));
  }
  while (blob.size() % 4) blob.push_back(0.0f);
  out.frac = blob.size();
  const int eband[kRnnBands] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 34, 40, 48, 60, 78, 100};
  std::vector<int32_t> band_of(484, kRnnBands - 1);
  blob.resize(blob.size() + 404, 0.0f);
  for (int b = 0; b < kRnnBands - 1; ++b) {
    const int size = (eband[b + 1] - eband[b]) << 2;
    for (int j = 0; j < size; ++j) {
      blob[out.frac + (eband[b] << 2) + j] = (float)j / (float)size;
      band_of[(eband[b] << 2) + j] = b;
    }
  }
  out.band_of_bin = blob.size();
  blob.resize(blob.size() + 484);
  std::memcpy(&blob[out.band_of_bin], band_of.data(), 484 * sizeof(int32_t));
  // the eleven matrices back as int8 (every entry of the f32 blob is a small integer), each word at the place the network
  // kernel reads it: dword [group][tile][lane] behind w4_matrix_offset(i), k padded to whole groups of 16 with zero weights
  out.w4.assign((size_t)w4_matrix_offset(11), 0u);
  for (int i = 0; i < 11; ++i) {
    const RnnLayerDims d = kRnnMatrixDims[i];
    const int tiles = d.n_pad / 16;
    for (int at = 0; at < w4_matrix_dwords(i); ++at) {
      const int lane = at % 64, t = at / 64 % tiles, g = at / 64 / tiles;
      uint32_t word = 0;
      for (int j = 0; j < 4; ++j) {
        const int k = 16 * g + 4 * j + (lane >> 4), n = 16 * t + (lane & 15);
        const int8_t v = k < d.k_pad ? (int8_t)blob[out.matrix[i] + (size_t)k * d.n_pad + n] : (int8_t)0;
        word |= (uint32_t)(uint8_t)v << (8 * j);
      }
      out.w4[(size_t)w4_matrix_offset(i) + at] = word;
    }
  }
  return out;
}

// The suppressor's settings, weights and device memory.  The buffers are owners (af_hip_resources.hpp): the engine that holds
// this object makes its device current, and synchronises it, before they are used or destroyed.
struct SuppressorHost {
  bool enabled = false;
  bool raw_protocol = false;
  float strength = 1.0f;
  RnnWeightsI8 weights;
  bool weights_dirty = true;
  // device side
  DeviceBuffer<float> d_blob;   // all f32 matrices + tables, one allocation
  DeviceBuffer<uint32_t> d_w4;  // the matrices as int8 in the network kernel's operand order (af_suppressor.h)
  RnnDeviceWeights dw{};
  SuppTables tables{};
  DeviceBuffer<float> d_state;  // [streams][SuppState::kCount]
  DeviceBuffer<float> d_xh;
  DeviceBuffer<float> d_ds;
  static constexpr int kXhBuffers = 4;    // model-input buffers: the pre-pass runs up to three windows ahead of the synthesis
  static constexpr int kSpecBuffers = kSuppSpecBuffers;  // spectrum / pitch-spectrum / record buffers: the analysis runs up to two windows ahead
  size_t xh_floats = 0;  // floats per model-input buffer
  size_t ws_cells = 0;   // (frame, stream) cells per spectrum / record buffer
  DeviceBuffer<float2> d_X, d_P;
  DeviceBuffer<SuppFrameRec> d_rec;
  int ws_frames = 0, ws_streams = 0;
  int last_xh_slot = -1, last_xh_frames = 0;  // the model-input buffer the last pre-pass wrote and its window's frames (test tap)

  SuppressorHost() { synthetic_weights(weights, 0x5EEDULL); }

  // weights_dirty stays set until both copies have been made: after a failure the next call sends everything again
  hipError_t upload() {
    const SuppressorBlob b = build_suppressor_blob(weights);
    if (hipError_t err = d_blob.reserve_exact(b.f32.size() * sizeof(float)); err != hipSuccess) return err;
    if (hipError_t err = hipMemcpy(d_blob, b.f32.data(), b.f32.size() * sizeof(float), hipMemcpyHostToDevice); err != hipSuccess) return err;
    if (hipError_t err = d_w4.reserve_exact(b.w4.size() * sizeof(uint32_t)); err != hipSuccess) return err;
    if (hipError_t err = hipMemcpy(d_w4, b.w4.data(), b.w4.size() * sizeof(uint32_t), hipMemcpyHostToDevice); err != hipSuccess) return err;
    dw.dense_w = d_blob + b.matrix[0];
    dw.dense_b = d_blob + b.bias[0];
    for (int g = 0; g < 3; ++g) {
      dw.vad_w[g] = d_blob + b.matrix[1 + g];
      dw.vad_b[g] = d_blob + b.bias[1 + g];
      dw.noise_w[g] = d_blob + b.matrix[4 + g];
      dw.noise_b[g] = d_blob + b.bias[4 + g];
      dw.den_w[g] = d_blob + b.matrix[7 + g];
      dw.den_b[g] = d_blob + b.bias[7 + g];
    }
    dw.out_w = d_blob + b.matrix[10];
    dw.out_b = d_blob + b.bias[10];
    dw.tansig = d_blob + b.tansig;
    dw.w4 = d_w4;
    tables.half_window = d_blob + b.half_window;
    tables.dct = d_blob + b.dct;
    tables.twiddle = reinterpret_cast<const float2 *>(d_blob + b.twiddle);
    tables.frac = d_blob + b.frac;
    tables.band_of_bin = reinterpret_cast<const int32_t *>(d_blob + b.band_of_bin);
    weights_dirty = false;
    return hipSuccess;
  }

  hipError_t reset_state(int n_streams) {
    std::vector<float> all((size_t)SuppState::kCount * n_streams, 0.0f);
    for (int s = 0; s < n_streams; ++s) all[(size_t)s * SuppState::kCount + SuppState::kSmoothedStrength] = 1.0f;  // rnnoise.rs:59
    if (hipError_t err = d_state.reserve_exact(all.size() * sizeof(float)); err != hipSuccess) return err;
    return hipMemcpy(d_state, all.data(), all.size() * sizeof(float), hipMemcpyHostToDevice);
  }

  // No-op when the frames fit; otherwise the five buffers are freed first and allocated exactly.  After a failure there is no
  // workspace (and no size is claimed), so the next call allocates again.
  hipError_t ensure_workspace(int n_streams, int frames) {
    if (frames <= ws_frames && n_streams == ws_streams) return hipSuccess;
    drop_workspace();
    const size_t cells = (size_t)frames * n_streams;
    // The windows of a call run as a pipeline (pre-pass | analysis | synthesis), so the buffers that cross a
    // stage boundary exist several times: the model input lives from the pre-pass to the synthesis (3 windows
    // in flight), spectra and frame records from the analysis to the synthesis (2), pitch spectra / resynthesised
    // frames from the network half of the synthesis to its resynthesis half (2).
    const size_t xh = (size_t)n_streams * (kPitchBuf + (size_t)frames * kRnnFrame);
    hipError_t err = d_xh.reserve_exact(sizeof(float) * kXhBuffers * xh);
    if (err == hipSuccess) err = d_X.reserve_exact(sizeof(float2) * kSpecBuffers * cells * kRnnFreq);
    if (err == hipSuccess) err = d_P.reserve_exact(sizeof(float2) * kSpecBuffers * cells * kRnnFreq);
    if (err == hipSuccess) err = d_rec.reserve_exact(sizeof(SuppFrameRec) * kSpecBuffers * cells);
    if (err == hipSuccess) err = d_ds.reserve_exact(sizeof(float) * cells * (kPitchBuf / 2));
    if (err != hipSuccess) {
      drop_workspace();
      return err;
    }
    xh_floats = xh;
    ws_cells = cells;
    ws_frames = frames;
    ws_streams = n_streams;
    return hipSuccess;
  }

  // The pointer fields of `sa` for window `index` of a call at pipeline depth `depth`: model-input buffer index % kXhBuffers,
  // spectrum / pitch-spectrum / record set index % depth, the single set of whitened pitch buffers, the state rows, and, behind
  // the call's first window, the history source: the buffer of the window before, whose rows hold `prev_frames` frames.
  void window_buffers(SuppArgs &sa, int64_t index, int depth, int64_t prev_frames) const {
    const size_t set = (size_t)(index % depth) * ws_cells;
    sa.xh = d_xh + (size_t)(index % kXhBuffers) * xh_floats;
    sa.X = d_X + set * kRnnFreq;
    sa.P = d_P + set * kRnnFreq;
    sa.ds = d_ds;
    sa.rec = d_rec + set;
    sa.state = d_state;
    if (index > 0) {  // history = tail of the previous window's buffer
      sa.xh_prev = d_xh + (size_t)((index - 1) % kXhBuffers) * xh_floats;
      sa.xh_prev_stride = kPitchBuf + prev_frames * kRnnFrame;
    }
  }

 private:
  void drop_workspace() {
    d_xh.release();
    d_ds.release();
    d_X.release();
    d_P.release();
    d_rec.release();
    xh_floats = ws_cells = 0;
    ws_frames = ws_streams = 0;
    last_xh_slot = -1;
    last_xh_frames = 0;
  }
};

}  // namespace af

