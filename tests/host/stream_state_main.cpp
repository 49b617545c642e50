// stream_state_main.cpp -- the canonical limiter ring of csrc/af_stream_state.h against a brute-force model of what the chain
// kernels do to the ring, the suffix maxima and the prefix maximum (af_kernels.hip "lookahead limiter"; the token-ring, quad
// and role kernels run the same update).  Stand-alone, host only: no HIP runtime, no device.
//
// For W in {2, 21, 97} and every pair of source and destination phases: drive a random sequence to the source phase, read
// the ring out oldest first, place it at the destination phase.  The rows must equal those of a model driven to the
// destination phase over the same last W inputs (silence before them), and the next 3 W limiter outputs must equal the
// source's own continuation bit for bit.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "af_stream_state.h"

namespace {

int failures = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      if (++failures <= 20) {                 \
        std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        std::printf(__VA_ARGS__);             \
        std::printf("\n");                    \
      }                                       \
    }                                         \
  } while (0)

// one stream of the kernels' limiter: the state rows and the per-sample update, statement for statement
struct Limiter {
  int W;
  std::vector<float> ring, suf;
  float prefix = 0.0f;
  double gain = 1.0;
  int64_t n = 0;  // the ENGINE's sample count: the ring position is n % W
  std::vector<float> seen;  // every input, for the brute-force window maximum
  explicit Limiter(int w) : W(w), ring((size_t)w, 0.0f), suf((size_t)w, 0.0f) {}

  float step(float xin, double ceil_lin, double rc, bool check_window) {
    const int j = (int)(n % W);
    const float ax = std::fabs(xin);
    const int jn = (j + 1 == W) ? 0 : j + 1;
    const float delayed = ring[(size_t)jn];
    const float sfx = (j + 1 < W) ? suf[(size_t)j + 1] : 0.0f;
    prefix = (j == 0) ? ax : std::fmax(prefix, ax);
    const double peak = (double)std::fmax(sfx, prefix);
    ring[(size_t)j] = xin;
    if (j + 1 == W) {
      float m = 0.0f;
      for (int k = W - 1; k >= 0; --k) {
        m = std::fmax(m, std::fabs(ring[(size_t)k]));
        suf[(size_t)k] = m;
      }
    }
    if (check_window) {  // what the block maxima stand for: the maximum over the last W inputs, this one included
      seen.push_back(xin);
      float m = 0.0f;
      for (int k = 0; k < W && k < (int)seen.size(); ++k) m = std::fmax(m, std::fabs(seen[seen.size() - 1 - (size_t)k]));
      CHECK(m == (float)peak, "W %d n %lld: window maximum %g, block maxima give %g", W, (long long)n, m, peak);
    }
    ++n;
    const double target = peak > ceil_lin ? ceil_lin / peak : 1.0;
    gain = target < gain ? target : rc * gain + (1.0 - rc) * target;
    double limited = (double)delayed * gain;
    limited = limited < -ceil_lin ? -ceil_lin : (limited > ceil_lin ? ceil_lin : limited);
    return (float)limited;
  }
};

uint64_t rng_state = 0x243F6A8885A308D3ull;
float rnd() {  // in [-1.6, 1.6], with exact zeros and runs of small values so that the maxima move
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  const uint32_t r = (uint32_t)(rng_state >> 33);
  if ((r & 15u) == 0) return 0.0f;
  const float u = (float)(r >> 8) / (float)(1u << 23) - 1.0f;
  return ((r & 7u) < 3u ? 0.05f : 1.6f) * u;
}

bool same_bits(const std::vector<float> &a, const std::vector<float> &b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}
bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }

void run(int W) {
  using namespace af::sstate;
  const double ceil_lin = 0.8413951416451951, rc = 0.99958;  // -1.5 dB, 50 ms at 48 kHz
  for (int ps = 0; ps < W; ++ps) {
    // the source: 3 W + ps inputs, phase ps
    Limiter src(W);
    std::vector<float> inputs;
    for (int t = 0; t < 3 * W + ps; ++t) {
      inputs.push_back(rnd());
      src.step(inputs.back(), ceil_lin, rc, ps < 3);
    }
    CHECK((int)(src.n % W) == ps, "source phase");
    // canonical form: oldest first == the last W inputs
    std::vector<float> canon((size_t)W);
    for (int c = 0; c < W; ++c) canon[(size_t)c] = src.ring[(size_t)ring_row(W, ps, c)];
    for (int c = 0; c < W; ++c)
      CHECK(same_bits(canon[(size_t)c], inputs[inputs.size() - (size_t)W + (size_t)c]), "W %d phase %d: canonical entry %d", W, ps, c);
    // the source's own next 3 W outputs
    std::vector<float> next;
    for (int t = 0; t < 3 * W; ++t) next.push_back(rnd());
    std::vector<float> want;
    {
      Limiter cont = src;
      for (float x : next) want.push_back(cont.step(x, ceil_lin, rc, false));
    }
    for (int pd = 0; pd < W; ++pd) {
      Limiter dst(W);
      dst.prefix = place_ring(
          W, pd, [&](int c) { return canon[(size_t)c]; }, [&](int row, float x) { dst.ring[(size_t)row] = x; },
          [&](int row, float m) { dst.suf[(size_t)row] = m; });
      dst.gain = src.gain;
      dst.n = (int64_t)7 * W + pd;  // any count at that phase
      // the model driven to the destination phase over the same last W inputs
      Limiter ref(W);
      for (int t = 0; t < pd; ++t) ref.step(0.0f, ceil_lin, rc, false);
      for (int c = 0; c < W; ++c) ref.step(canon[(size_t)c], ceil_lin, rc, false);
      CHECK((int)(ref.n % W) == pd, "reference phase");
      CHECK(same_bits(dst.ring, ref.ring), "W %d %d -> %d: ring rows", W, ps, pd);
      CHECK(same_bits(dst.suf, ref.suf), "W %d %d -> %d: suffix rows", W, ps, pd);
      CHECK(same_bits(dst.prefix, ref.prefix), "W %d %d -> %d: prefix %g, model %g", W, ps, pd, dst.prefix, ref.prefix);
      // same phase: the rows the limiter reads before it rewrites them are the source's own
      if (pd == ps) {
        CHECK(same_bits(dst.ring, src.ring), "W %d phase %d: ring rows at the source's phase", W, ps);
        for (int k = ps + 1; k < W; ++k) CHECK(same_bits(dst.suf[(size_t)k], src.suf[(size_t)k]), "W %d phase %d: suffix row %d", W, ps, k);
        if (ps > 0) CHECK(same_bits(dst.prefix, src.prefix), "W %d phase %d: prefix", W, ps);
      }
      for (size_t t = 0; t < next.size(); ++t) {
        const float got = dst.step(next[t], ceil_lin, rc, false);
        if (!same_bits(got, want[t])) {
          CHECK(false, "W %d %d -> %d: output %zu is %.9g, the source continues with %.9g", W, ps, pd, t, got, want[t]);
          break;
        }
      }
    }
  }
}

void layout() {
  using namespace af::sstate;
  Shape s{};
  s.rows64 = af::f64_field_count(0, 0);
  s.rows32 = af::kF32Fixed + 97;
  CHECK(blob_bytes(s) == ((72u + 8u * (size_t)s.rows64 + 4u * (size_t)s.rows32 + 7u) & ~(size_t)7u), "plain blob size");
  s.gate_plane = 1;
  s.suppressor = 1;
  CHECK(blob_f32_offset(s) == 72u + 8u * ((size_t)s.rows64 + 11u), "f32 rows behind the gate row");
  CHECK(blob_supp_offset(s) == blob_f32_offset(s) + 4u * (size_t)s.rows32, "suppressor row behind the f32 rows");
  CHECK(blob_bytes(s) >= blob_supp_offset(s) + 4u * 2580u && blob_bytes(s) % 8 == 0, "whole blob");
  CHECK(stage_bytes(s, 5) == 5u * (8u * ((size_t)s.rows64 + 11u) + 4u * (size_t)s.rows32 + 4u * 2580u), "staging size");
  const Geometry g = geometry(300, 10, true, true);
  CHECK(g.chunks == 2 && g.a_blocks == 20 && g.b_blocks == 2 && g.c_blocks == 300 * 11 && g.total() == 22 + 3300, "geometry");
}

}  // namespace

int main() {
  layout();
  for (int W : {2, 21, 97}) run(W);
  // W = 1 (no lookahead): one row, phase always 0
  run(1);
  if (failures) {
    std::printf("stream_state: %d failures\n", failures);
    return 1;
  }
  std::printf("stream_state: ok\n");
  return 0;
}
