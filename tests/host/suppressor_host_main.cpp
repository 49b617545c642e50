// Stand-alone test of csrc/af_suppressor_host.hpp: SuppressorHost's device memory against the fake HIP runtime of
// fake_hip_runtime.hpp (every allocation that can fail, failed in turn), its buffer-set accessor against the expressions the
// pipeline used before there was one, and the pure host builder of the weight and table blob against the layouts written out
// here independently.  Built with -fsanitize=address,undefined by tests/test_host_resources.py.
#include "af_suppressor_host.hpp"
#include "fake_hip_runtime.hpp"

using af::SuppressorHost;
using af::SuppState;

// the five workspace allocations for `streams` x `frames`, in the order they are made: model input, spectra, pitch spectra,
// records, whitened pitch buffers
static std::vector<size_t> workspace_bytes(size_t streams, size_t frames) {
  const size_t cells = streams * frames;
  return {4 * (4 * streams * (1728 + 480 * frames)), 8 * (3 * cells * 481), 8 * (3 * cells * 481), sizeof(af::SuppFrameRec) * 3 * cells,
          4 * (cells * 864)};
}

static void test_workspace() {
  fake::reset();
  {
    SuppressorHost h;
    CHECK(h.ensure_workspace(3, 4) == hipSuccess);
    CHECK(fake::calls == 5 && fake::alloc_log == workspace_bytes(3, 4) && fake::device.size() == 5);
    CHECK(h.ws_frames == 4 && h.ws_streams == 3 && h.ws_cells == 12 && h.xh_floats == 3 * (1728 + 4 * 480));
    CHECK(h.ensure_workspace(3, 4) == hipSuccess && h.ensure_workspace(3, 2) == hipSuccess && fake::calls == 5);  // they fit
    CHECK(h.ws_frames == 4);
    CHECK(h.ensure_workspace(3, 7) == hipSuccess);
    CHECK(fake::calls == 15 && fake::device_frees == 5 && fake::device.size() == 5);
    CHECK(std::vector<size_t>(fake::alloc_log.begin() + 5, fake::alloc_log.end()) == workspace_bytes(3, 7));
    CHECK(h.ws_frames == 7 && h.ws_cells == 21 && h.xh_floats == 3 * (1728 + 7 * 480));
    CHECK(h.ensure_workspace(2, 7) == hipSuccess && fake::device_frees == 10 && h.ws_streams == 2);  // another stream count: again
  }
  CHECK(fake::nothing_live());
}

// the k-th of the five allocations fails, with and without a workspace to grow from; `retry`: the call is repeated
static void test_workspace_failures() {
  for (int grown = 0; grown < 2; ++grown)
    for (int k = 1; k <= 5; ++k)
      for (int retry = 0; retry < 2; ++retry) {
        fake::reset();
        {
          SuppressorHost h;
          if (grown) CHECK(h.ensure_workspace(3, 2) == hipSuccess);
          fake::fail_at = fake::fallible + k;
          CHECK(h.ensure_workspace(3, 4) == hipErrorOutOfMemory);
          CHECK(fake::device.empty());  // nothing is kept half-way ...
          CHECK(h.ws_frames == 0 && h.ws_streams == 0 && h.ws_cells == 0 && h.xh_floats == 0);  // ... and no size is claimed
          CHECK(!h.d_xh && !h.d_X && !h.d_P && !h.d_rec && !h.d_ds);
          if (retry) {
            fake::alloc_log.clear();
            CHECK(h.ensure_workspace(3, 4) == hipSuccess);
            CHECK(fake::alloc_log == workspace_bytes(3, 4) && fake::device.size() == 5 && h.ws_frames == 4 && h.ws_cells == 12);
          }
        }
        CHECK(fake::nothing_live());
      }
}

static void test_reset_state() {
  fake::reset();
  {
    SuppressorHost h;
    CHECK(h.reset_state(3) == hipSuccess);
    CHECK(fake::alloc_log == std::vector<size_t>{sizeof(float) * SuppState::kCount * 3});
    const float *rows = h.d_state;
    for (int s = 0; s < 3; ++s)
      for (int i = 0; i < SuppState::kCount; ++i) CHECK(rows[s * SuppState::kCount + i] == (i == SuppState::kSmoothedStrength ? 1.0f : 0.0f));
    h.d_state[5] = 3.0f;
    CHECK(h.reset_state(3) == hipSuccess && fake::alloc_log.size() == 1 && h.d_state[5] == 0.0f);  // the same buffer, written again
    fake::fail_at = fake::fallible + 1;
    SuppressorHost other;
    CHECK(other.reset_state(3) != hipSuccess && !other.d_state);
  }
  CHECK(fake::nothing_live());
}

// every fallible call of upload() (allocation and copy of the blob, allocation and copy of the int8 matrices) fails in turn
static void test_upload_failures() {
  long fallible_calls = 0;
  for (long k = 0; k == 0 || k <= fallible_calls; ++k) {  // k = 0: the run that counts them
    fake::reset();
    {
      SuppressorHost h;
      CHECK(h.weights_dirty);
      if (k) fake::fail_at = k;
      const hipError_t err = h.upload();
      if (k == 0) {
        fallible_calls = fake::fallible;
        CHECK(err == hipSuccess && fallible_calls == 4);
      } else {
        CHECK(err != hipSuccess && h.weights_dirty);
        fake::fail_at = 0;
        CHECK(h.upload() == hipSuccess);  // the next call sends everything again
      }
      CHECK(!h.weights_dirty && fake::device.size() == 2);
      const af::SuppressorBlob b = af::build_suppressor_blob(h.weights);
      CHECK(fake::device.at(h.d_blob.get()) == b.f32.size() * sizeof(float) && fake::device.at(h.d_w4.get()) == b.w4.size() * sizeof(uint32_t));
      CHECK(std::memcmp(h.d_blob, b.f32.data(), b.f32.size() * sizeof(float)) == 0);
      CHECK(std::memcmp(h.d_w4, b.w4.data(), b.w4.size() * sizeof(uint32_t)) == 0);
      CHECK(h.dw.dense_w == h.d_blob + b.matrix[0] && h.dw.den_b[2] == h.d_blob + b.bias[9] && h.dw.out_w == h.d_blob + b.matrix[10]);
      CHECK(h.dw.w4 == h.d_w4.get() && h.dw.tansig == h.d_blob + b.tansig && h.tables.frac == h.d_blob + b.frac);
      const long calls = fake::calls;
      h.weights_dirty = true;
      CHECK(h.upload() == hipSuccess && fake::calls == calls + 2 && fake::device.size() == 2);  // the buffers fit: two copies
    }
    CHECK(fake::nothing_live());
    {
      SuppressorHost h;  // destroyed right after the failure
      if (k) fake::fail_at = fake::fallible + k;
      (void)h.upload();
    }
    CHECK(fake::nothing_live());
  }
}

// The pointers of window `index` at pipeline depth `depth`, as run_suppressor_pipeline computed them before SuppressorHost had
// an accessor (the expressions of its `window_args`, with `supp` for `e->supp`).
static void test_window_buffers() {
  fake::reset();
  {
    SuppressorHost supp;
    CHECK(supp.ensure_workspace(3, 4) == hipSuccess && supp.reset_state(3) == hipSuccess);
    constexpr int kXh = SuppressorHost::kXhBuffers;
    const long calls = fake::calls;
    for (int depth = 2; depth <= 3; ++depth)
      for (int64_t index = 0; index < 10; ++index) {
        const int64_t prev_frames = 1 + index % 4;
        af::SuppArgs sa{};
        supp.window_buffers(sa, index, depth, prev_frames);
        CHECK(sa.xh == supp.d_xh + (size_t)(index % kXh) * supp.xh_floats);
        CHECK(sa.X == supp.d_X + (size_t)(index % depth) * supp.ws_cells * af::kRnnFreq);
        CHECK(sa.P == supp.d_P + (size_t)(index % depth) * supp.ws_cells * af::kRnnFreq);
        CHECK(sa.ds == supp.d_ds);
        CHECK(sa.rec == supp.d_rec + (size_t)(index % depth) * supp.ws_cells);
        CHECK(sa.state == supp.d_state);
        if (index > 0) {
          CHECK(sa.xh_prev == supp.d_xh + (size_t)((index - 1) % kXh) * supp.xh_floats);
          CHECK(sa.xh_prev_stride == af::kPitchBuf + prev_frames * af::kRnnFrame);
        } else {
          CHECK(sa.xh_prev == nullptr && sa.xh_prev_stride == 0);
        }
        // every set lies inside its allocation
        CHECK((size_t)(sa.xh - supp.d_xh) + supp.xh_floats <= supp.d_xh.bytes() / sizeof(float));
        CHECK((size_t)(sa.X - supp.d_X) + supp.ws_cells * af::kRnnFreq <= supp.d_X.bytes() / sizeof(float2));
        CHECK((size_t)(sa.rec - supp.d_rec) + supp.ws_cells <= supp.d_rec.bytes() / sizeof(af::SuppFrameRec));
      }
    CHECK(fake::calls == calls);
  }
  CHECK(fake::nothing_live());
  fake::reset();
  { SuppressorHost never_used; }
  CHECK(fake::calls == 0);
}

// ---- the builder.  The model's layout (af_suppressor_host.hpp, RnnWeightsI8): dense [in][out]; GRU [in][3 units] and
// [units][3 units], gate order z | r | h, bias [3 units].
struct Source { const int8_t *w, *u, *b; int gate, gates; };

static void test_blob(const af::RnnWeightsI8 &w) {
  const af::SuppressorBlob blob = af::build_suppressor_blob(w);
  const Source src[11] = {{w.input_dense_w, nullptr, w.input_dense_b, 0, 1},
                          {w.vad_gru_w, w.vad_gru_u, w.vad_gru_b, 0, 3}, {w.vad_gru_w, w.vad_gru_u, w.vad_gru_b, 1, 3}, {w.vad_gru_w, w.vad_gru_u, w.vad_gru_b, 2, 3},
                          {w.noise_gru_w, w.noise_gru_u, w.noise_gru_b, 0, 3}, {w.noise_gru_w, w.noise_gru_u, w.noise_gru_b, 1, 3}, {w.noise_gru_w, w.noise_gru_u, w.noise_gru_b, 2, 3},
                          {w.denoise_gru_w, w.denoise_gru_u, w.denoise_gru_b, 0, 3}, {w.denoise_gru_w, w.denoise_gru_u, w.denoise_gru_b, 1, 3}, {w.denoise_gru_w, w.denoise_gru_u, w.denoise_gru_b, 2, 3},
                          {w.denoise_out_w, nullptr, w.denoise_out_b, 0, 1}};
  const int dims[11][5] = {{42, 0, 44, 24, 32}, {24, 24, 48, 24, 32}, {24, 24, 48, 24, 32}, {24, 24, 48, 24, 32}, {90, 48, 140, 48, 48}, {90, 48, 140, 48, 48},
                           {90, 48, 140, 48, 48}, {114, 96, 212, 96, 96}, {114, 96, 212, 96, 96}, {114, 96, 212, 96, 96}, {96, 0, 96, 22, 32}};
  size_t at = 0;   // where the next part of the f32 blob must start: the parts are back to back
  size_t at4 = 0;  // ... and of the int8 words
  for (int i = 0; i < 11; ++i) {
    const int k_in = dims[i][0], k_rec = dims[i][1], k_pad = dims[i][2], n_out = dims[i][3], n_pad = dims[i][4];
    const Source &s = src[i];
    const int row = s.gates * n_out, col0 = s.gate * n_out;
    // the integers of the matrix, padding included
    std::vector<int> m((size_t)k_pad * n_pad, 0);
    for (int k = 0; k < k_in; ++k)
      for (int n = 0; n < n_out; ++n) m[(size_t)k * n_pad + n] = s.w[k * row + col0 + n];
    for (int k = 0; k < k_rec; ++k)
      for (int n = 0; n < n_out; ++n) m[(size_t)(k_in + k) * n_pad + n] = s.u[k * row + col0 + n];
    CHECK(blob.matrix[i] == at);
    for (int k = 0; k < k_pad; ++k)
      for (int n = 0; n < n_pad; ++n) CHECK(blob.f32[blob.matrix[i] + (size_t)k * n_pad + n] == (float)m[(size_t)k * n_pad + n]);
    at += (size_t)k_pad * n_pad;
    CHECK(blob.bias[i] == at);
    for (int n = 0; n < n_pad; ++n) CHECK(blob.f32[blob.bias[i] + n] == (n < n_out ? (float)s.b[col0 + n] : 0.0f));
    at += n_pad;
    // the operand order of the network kernel: rows in groups of 16, columns in tiles of 16; lane (k % 4) * 16 + n % 16 of
    // a (group, tile) holds rows 4 j + k % 4 of the group in its bytes j = 0..3; rows past k_pad are zero weights
    CHECK(af::w4_matrix_offset(i) == (int)at4);
    const int groups = (k_pad + 15) / 16, tiles = n_pad / 16;
    for (int k = 0; k < 16 * groups; ++k)
      for (int n = 0; n < n_pad; ++n) {
        const int g = k / 16, j = k % 16 / 4, lane = (k % 4) * 16 + n % 16, t = n / 16;
        const uint32_t word = blob.w4[at4 + ((size_t)g * tiles + t) * 64 + lane];
        CHECK((int)(int8_t)(word >> (8 * j) & 0xffu) == (k < k_pad ? m[(size_t)k * n_pad + n] : 0));
      }
    at4 += (size_t)groups * tiles * 64;
  }
  CHECK(blob.w4.size() == at4);
  // the tables, each a multiple of four floats behind the one before, padding zero
  const std::vector<float> &f = blob.f32;
  const double pi = 3.14159265358979323846;
  CHECK(blob.tansig == at && blob.half_window == at + 204 && blob.dct == at + 204 + 480 && blob.twiddle == blob.dct + 484);
  CHECK(blob.frac == blob.twiddle + 1920 && blob.band_of_bin == blob.frac + 404 && f.size() == blob.band_of_bin + 484);
  CHECK(f[blob.tansig] == 0.0f && f[blob.tansig + 100] == (float)std::tanh(0.04 * 100) && f[blob.tansig + 200] == (float)std::tanh(0.04 * 200));
  for (int i = 201; i < 204; ++i) CHECK(f[blob.tansig + i] == 0.0f);
  for (int i : {0, 1, 240, 479}) {
    const double sn = std::sin(.5 * pi * (i + .5) / 480);
    CHECK(f[blob.half_window + i] == (float)std::sin(.5 * pi * sn * sn));
  }
  CHECK(f[blob.dct] == (float)std::sqrt(.5) && f[blob.dct + 21 * 22] == (float)(std::cos(0.0) * std::sqrt(.5)));
  CHECK(f[blob.dct + 1] == (float)std::cos(.5 * pi / 22) && f[blob.dct + 21 * 22 + 21] == (float)std::cos(21.5 * 21 * pi / 22));
  for (int i : {0, 1, 240, 959}) {
    CHECK(f[blob.twiddle + 2 * i] == (float)std::cos(-2.0 * pi * i / 960));
    CHECK(f[blob.twiddle + 2 * i + 1] == (float)std::sin(-2.0 * pi * i / 960));
  }
  // bands start at bins 4 x {0 1 2 .. 8 10 12 14 16 20 24 28 34 40 48 60 78 100}; bins from 400 on belong to no band
  CHECK(f[blob.frac] == 0.0f && f[blob.frac + 1] == 0.25f && f[blob.frac + 3] == 0.75f && f[blob.frac + 4] == 0.0f);
  CHECK(f[blob.frac + 33] == 1.0f / 8.0f && f[blob.frac + 399] == 87.0f / 88.0f);
  for (int i = 400; i < 404; ++i) CHECK(f[blob.frac + i] == 0.0f);
  int32_t band[484];
  std::memcpy(band, &f[blob.band_of_bin], sizeof band);
  CHECK(band[0] == 0 && band[3] == 0 && band[4] == 1 && band[31] == 7 && band[32] == 8 && band[39] == 8 && band[40] == 9);
  CHECK(band[311] == 19 && band[312] == 20 && band[399] == 20 && band[400] == 21 && band[483] == 21);
}

int main() {
  test_workspace();
  test_workspace_failures();
  test_reset_state();
  test_upload_failures();
  test_window_buffers();
  af::RnnWeightsI8 w;
  af::synthetic_weights(w, 0x5EEDULL);
  test_blob(w);
  int8_t *bytes = reinterpret_cast<int8_t *>(&w);
  for (size_t i = 0; i < sizeof w; ++i) bytes[i] = (int8_t)(i * 37 + 11);  // neighbours differ
  test_blob(w);
  std::puts("suppressor host: ok");
  return 0;
}
