// af_stream_state.h -- the per-stream lifecycle (restart, export, import of single streams of a live engine): the blob
// layout, the canonical form of the limiter's ring, and the launch geometry, shared by the host side (af_api.cpp), the
// kernels (af_stream_state.hip) and the stand-alone host check (tests/host/stream_state_main.cpp).  Plain C++: no HIP
// header is needed to include it.
//
// A stream's state is its column of the two chain planes (af_device.h), its gate row and its suppressor row.  All of it is
// per-stream by construction but for three f32 fields that are addressed by the ENGINE's absolute sample count n (every
// stream of an engine advances in lock step):
//   * the limiter's delay ring: input n lives in ring row n % W            (W = lookahead + 1)
//   * the van-Herk suffix maxima of the last complete block of W inputs    (block = inputs [n - n % W - W, n - n % W))
//   * the running prefix maximum of the block in progress                  (inputs [n - n % W, n))
// The blob therefore stores the last W limiter inputs OLDEST FIRST and neither maxima; an import places the ring at the
// destination's phase p = n_dst % W and recomputes both.  They are maxima of |x| over inputs that all lie inside the last
// W, wherever the limiter reads them before it overwrites them, so the continuation is bit-exact.  (The true-peak
// histories are stored oldest first by every kernel already, and the loudness meter's ring position is a per-stream row.)
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "af_device.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AF_SS_HD __host__ __device__
#else
#define AF_SS_HD
#endif

namespace af {
namespace sstate {

constexpr uint32_t kMagic = 0x53534641u;  // "AFSS", little endian
constexpr uint32_t kVersion = 1;
// a suppressor row (SuppState::kCount floats) and a gate row (kGateFields words) of af_suppressor.h, which needs the HIP
// headers; af_stream_state.hip asserts that they agree
constexpr int kSuppRowFloats = 2580, kGateRowWords = 11, kSuppStrengthField = 2579;

// What must agree between the blob and the slot it is imported into: the sample rate, the control block, and the shape of
// the slot's preset and of the engine's planes.  Parameter VALUES are not part of it.
struct Shape {
  double sample_rate;
  int32_t control_block;
  int32_t n_eq_sections;   // of the slot's preset
  int32_t lookahead;       // limiter lookahead of the slot's preset, samples
  int32_t meter_slots;     // loudness-meter slots of the slot's preset (0: no auto-makeup)
  uint32_t stage_flags;    // kStageMask bits of ChainParams::flags, kStageAutoMakeup
  int32_t suppressor;      // 1: a suppressor row follows
  int32_t gate_plane;      // 1: a gate row follows
  int32_t live_rows;       // 1: the f64 rows end with live control's 15 pending dynamic-EQ rows
  int32_t rows64;          // f64 rows stored (the engine's plane height)
  int32_t rows32;          // f32 rows stored: kF32Fixed + the engine's ring capacity (its largest W)
};
constexpr uint32_t kStageMask = kFlagDeesser | kFlagEq | kFlagCompressor | kFlagLimiter | kFlagEqBeforeDeesser |
                                kFlagInputScrub | kFlagInputClamp | kFlagDcBlock | kFlagPreHighpass;
constexpr uint32_t kStageAutoMakeup = 1u << 16;

struct BlobHeader {
  uint32_t magic, version;
  uint32_t header_bytes, blob_bytes;
  Shape shape;
  int64_t samples;  // the stream's own sample count (since its last restart, or carried over an import)
};
static_assert(sizeof(Shape) == 48 && sizeof(BlobHeader) == 72, "blob header layout");

// Blob body, behind the header: [rows64] f64 | [kGateFields] int64 (gate_plane) | [rows32] f32 | [SuppState::kCount] f32
// (suppressor), padded to 8 bytes.  The f32 rows are the kF32Fixed fixed rows (kLimPrefix stored as 0) followed by the
// canonical ring: the preset's W inputs oldest first, then zeros up to the engine's capacity.
AF_SS_HD inline int words64(const Shape &s) { return s.rows64 + (s.gate_plane ? kGateRowWords : 0); }
AF_SS_HD inline size_t blob_bytes(const Shape &s) {
  const size_t b = sizeof(BlobHeader) + 8u * (size_t)words64(s) + 4u * (size_t)s.rows32 +
                   (s.suppressor ? 4u * (size_t)kSuppRowFloats : 0u);
  return (b + 7u) & ~(size_t)7u;
}
AF_SS_HD inline size_t blob_f32_offset(const Shape &s) { return sizeof(BlobHeader) + 8u * (size_t)words64(s); }
AF_SS_HD inline size_t blob_supp_offset(const Shape &s) { return blob_f32_offset(s) + 4u * (size_t)s.rows32; }

// The device staging buffer of a transfer of n streams is FIELD major, so that lanes over the stream list read and write
// consecutive addresses on both sides: [words64][n] 8-byte words | [rows32][n] f32 | [n][SuppState::kCount] f32.  The host
// transposes between it and the blobs.
AF_SS_HD inline size_t stage_f32_offset(const Shape &s, int64_t n) { return 8u * (size_t)words64(s) * (size_t)n; }
AF_SS_HD inline size_t stage_supp_offset(const Shape &s, int64_t n) { return stage_f32_offset(s, n) + 4u * (size_t)s.rows32 * (size_t)n; }
AF_SS_HD inline size_t stage_bytes(const Shape &s, int64_t n) {
  return stage_supp_offset(s, n) + (s.suppressor ? 4u * (size_t)kSuppRowFloats * (size_t)n : 0u);
}

// ---- the canonical ring ----------------------------------------------------------------------------------------------
// Canonical entry c (0 = oldest of the last W inputs, W - 1 = newest) of an engine at phase p = n % W lives in ring row
// (p + c) % W: the newest input n - 1 is in row (p - 1) % W, the oldest, n - W, in row p -- the row the next input overwrites.
AF_SS_HD inline int ring_row(int W, int p, int c) {
  const int r = p + c;
  return r >= W ? r - W : r;
}

// Place canonical inputs get(c) at phase p: put_ring(row, x) for the W ring rows, put_suffix(row, m) for the W suffix rows;
// returns the prefix maximum.
//   suffix[k] = max |x| over rows k .. W - 1 of the last complete block, whose row k holds canonical entry k - p.  Rows
//     k > p are the ones the limiter still reads (at step j it reads suffix[j + 1], j >= p).  Rows k < p reach back before
//     the last W inputs; they are never read before the block in progress completes and rewrites all of them, and get what
//     an engine would hold that had seen silence before those W inputs.
//   prefix = max |x| of the block in progress, canonical entries W - p .. W - 1; at p = 0 no block is in progress and the
//     value (overwritten by the next input) is that of the block just completed.
// fmaxf over magnitudes is exact and order-free, so these equal the kernels' running values bit for bit.
template <class Get, class PutRing, class PutSuffix>
AF_SS_HD inline float place_ring(int W, int p, Get get, PutRing put_ring, PutSuffix put_suffix) {
  for (int c = 0; c < W; ++c) put_ring(ring_row(W, p, c), get(c));
  float m = 0.0f;
  for (int k = W - 1; k >= 0; --k) {
    if (k >= p) m = fmaxf(m, fabsf(get(k - p)));
    put_suffix(k, m);
  }
  float prefix = 0.0f;
  for (int c = (p == 0 ? 0 : W - p); c < W; ++c) prefix = fmaxf(prefix, fabsf(get(c)));
  return prefix;
}

// ---- device side: one entry of the stream list, and the launch geometry ----------------------------------------------
struct Slot {
  int32_t stream;
  int32_t preset;  // restart: which prototype column
  int32_t W;       // lookahead + 1 of the slot's preset
  int32_t phase;   // engine samples % W
};

constexpr int kBlock = 256;  // threads per workgroup, all three kernels
// Work is cut into three regions of a 1-D grid:
//   A  plane rows: one workgroup per (row, 256 consecutive list entries); lane = list entry, so a sorted list of
//      neighbouring slots reads and writes consecutive plane addresses ([field][stream])
//   B  import only, the limiter ring: one lane per list entry walks its W canonical inputs (the suffix maxima are a running
//      maximum); every step of the walk is again consecutive across lanes on both sides
//   C  suppressor rows ([stream][field]): one workgroup per (list entry, 256 consecutive fields); lane = field
struct Geometry {
  int32_t chunks;  // ceil(n / kBlock)
  int32_t a_rows, a_blocks, b_blocks, c_per_entry, c_blocks;
  AF_SS_HD int64_t total() const { return (int64_t)a_blocks + b_blocks + c_blocks; }
};
AF_SS_HD inline Geometry geometry(int32_t n, int32_t plane_rows, bool ring_walk, bool suppressor) {
  Geometry g;
  g.chunks = (n + kBlock - 1) / kBlock;
  g.a_rows = plane_rows;
  g.a_blocks = plane_rows * g.chunks;
  g.b_blocks = ring_walk ? g.chunks : 0;
  g.c_per_entry = (kSuppRowFloats + kBlock - 1) / kBlock;
  g.c_blocks = suppressor ? n * g.c_per_entry : 0;
  return g;
}

}  // namespace sstate
}  // namespace af
