// af_stream_state_host.hpp -- host side of the per-stream lifecycle behind the entry points of af_api.cpp: the kernels'
// arguments and launchers (af_stream_state.hip), the checks that need no device, and the transposition between the
// field-major staging buffer and the caller's blobs.  Header only apart from the three launchers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "af_hip_resources.hpp"
#include "af_stream_state.h"

namespace af {
namespace sstate {

// the engine's per-stream state on the device
struct PlaneView {
  double *st64;    // [rows64][n_streams]
  float *st32;     // [rows32_plane][n_streams]
  int64_t *gate;   // [kGateRowWords][n_streams], or null: the engine has no gate plane
  float *supp;     // [n_streams][kSuppRowFloats], or null: the suppressor is off
  int32_t n_streams, rows64, rows32_plane, ring_cap;  // rows32_plane = kF32Fixed + 2 * ring_cap
};
struct RestartArgs {
  PlaneView v;
  const Slot *slots;      // device, [n]
  const double *proto64;  // device, [n_presets][rows64]: upload_initial_state's rows
  const float *proto32;   // device, [n_presets][kF32Fixed]
  int32_t n, n_presets;
  Geometry g;             // filled by the launcher
};
struct TransferArgs {
  PlaneView v;
  const Slot *slots;      // device, [n]
  int64_t *stage64;       // device staging (af_stream_state.h): [words64][n]
  float *stage32;         // [rows32][n]
  float *stage_supp;      // [n][kSuppRowFloats], or null with the suppressor off
  int32_t n, words64, rows32;
  Geometry g;
};
hipError_t launch_restart(RestartArgs a, hipStream_t stream);
hipError_t launch_export(TransferArgs a, hipStream_t stream);
hipError_t launch_import(TransferArgs a, hipStream_t stream);

// What an engine keeps for the lifecycle: the switch, each stream's own origin on the engine's sample axis (its sample count
// is the engine's minus this; an import may make it negative), the device staging buffer and the pinned slots lists,
// prototype rows and blobs travel through.
struct Lifecycle {
  bool enabled = false;
  std::vector<int64_t> origin;  // empty: every stream started with the engine
  DeviceBuffer<unsigned char> d_stage;
  PinnedSlots<2> stager;
  void clear() { origin.clear(); }
  int64_t origin_of(int32_t s) const { return origin.empty() ? 0 : origin[(size_t)s]; }
  void set_origin(int32_t s, int64_t v, int32_t n_streams) {
    if (origin.empty()) origin.assign((size_t)n_streams, 0);
    origin[(size_t)s] = v;
  }
};

// "" when `streams` is a list of n distinct indices below n_streams, else the message
inline std::string check_list(const int32_t *streams, int32_t n, int32_t n_streams) {
  char buf[160];
  if (n < 0) return "the stream count is negative";
  if (n > 0 && !streams) return "the stream list is null";
  std::vector<char> seen((size_t)n_streams, 0);
  for (int32_t i = 0; i < n; ++i) {
    if (streams[i] < 0 || streams[i] >= n_streams) {
      std::snprintf(buf, sizeof buf, "stream list entry %d is %d: out of range for %d streams", i, streams[i], n_streams);
      return buf;
    }
    if (seen[(size_t)streams[i]]) {
      std::snprintf(buf, sizeof buf, "stream list entry %d repeats stream %d: the list must hold distinct streams", i, streams[i]);
      return buf;
    }
    seen[(size_t)streams[i]] = 1;
  }
  return "";
}

// "" when a blob's header fits a slot of shape `want`, else a message that names the first field that does not
inline std::string check_header(const BlobHeader &h, const Shape &want) {
  char buf[200];
  auto bad = [&](const char *field, double got, double need) {
    std::snprintf(buf, sizeof buf, "stream state blob: %s is %.17g, the destination slot has %.17g", field, got, need);
    return std::string(buf);
  };
  if (h.magic != kMagic) return bad("magic", h.magic, kMagic);
  if (h.version != kVersion) return bad("version", h.version, kVersion);
  if (h.header_bytes != sizeof(BlobHeader)) return bad("header_bytes", h.header_bytes, (double)sizeof(BlobHeader));
  const Shape &s = h.shape;
  if (!(s.sample_rate == want.sample_rate)) return bad("sample_rate", s.sample_rate, want.sample_rate);
  if (s.control_block != want.control_block) return bad("control_block", s.control_block, want.control_block);
  if (s.n_eq_sections != want.n_eq_sections) return bad("n_eq_sections", s.n_eq_sections, want.n_eq_sections);
  if (s.lookahead != want.lookahead) return bad("lookahead", s.lookahead, want.lookahead);
  if (s.meter_slots != want.meter_slots) return bad("meter_slots", s.meter_slots, want.meter_slots);
  if (s.stage_flags != want.stage_flags) return bad("stage_flags", s.stage_flags, want.stage_flags);
  if (s.suppressor != want.suppressor) return bad("suppressor", s.suppressor, want.suppressor);
  if (s.gate_plane != want.gate_plane) return bad("gate_plane", s.gate_plane, want.gate_plane);
  if (s.live_rows != want.live_rows) return bad("live_rows", s.live_rows, want.live_rows);
  if (s.rows64 != want.rows64) return bad("rows64", s.rows64, want.rows64);
  if (s.rows32 != want.rows32) return bad("rows32", s.rows32, want.rows32);
  if (h.blob_bytes != blob_bytes(want)) return bad("blob_bytes", h.blob_bytes, (double)blob_bytes(want));
  return "";
}

// staging buffer (host copy) -> n blobs of blob_bytes(shapes[i]) each (all equal: the engine's size), `stride` apart
inline void stage_to_blobs(const unsigned char *stage, int32_t n, const std::vector<Shape> &shapes, const std::vector<int64_t> &samples,
                           unsigned char *blobs, size_t stride) {
  for (int32_t i = 0; i < n; ++i) {
    const Shape &s = shapes[(size_t)i];
    unsigned char *b = blobs + (size_t)i * stride;
    std::memset(b, 0, blob_bytes(s));
    BlobHeader h{};
    h.magic = kMagic;
    h.version = kVersion;
    h.header_bytes = (uint32_t)sizeof(BlobHeader);
    h.blob_bytes = (uint32_t)blob_bytes(s);
    h.shape = s;
    h.samples = samples[(size_t)i];
    std::memcpy(b, &h, sizeof h);
    const int w64 = words64(s);
    for (int r = 0; r < w64; ++r) std::memcpy(b + sizeof h + 8u * (size_t)r, stage + 8u * ((size_t)r * n + i), 8);
    const unsigned char *s32 = stage + stage_f32_offset(s, n);
    for (int r = 0; r < s.rows32; ++r) std::memcpy(b + blob_f32_offset(s) + 4u * (size_t)r, s32 + 4u * ((size_t)r * n + i), 4);
    if (s.suppressor)
      std::memcpy(b + blob_supp_offset(s), stage + stage_supp_offset(s, n) + 4u * (size_t)kSuppRowFloats * i, 4u * (size_t)kSuppRowFloats);
  }
}

// ... and back (the headers were checked)
inline void blobs_to_stage(const unsigned char *blobs, size_t stride, int32_t n, const Shape &s, unsigned char *stage) {
  const int w64 = words64(s);
  unsigned char *s32 = stage + stage_f32_offset(s, n);
  for (int32_t i = 0; i < n; ++i) {
    const unsigned char *b = blobs + (size_t)i * stride;
    for (int r = 0; r < w64; ++r) std::memcpy(stage + 8u * ((size_t)r * n + i), b + sizeof(BlobHeader) + 8u * (size_t)r, 8);
    for (int r = 0; r < s.rows32; ++r) std::memcpy(s32 + 4u * ((size_t)r * n + i), b + blob_f32_offset(s) + 4u * (size_t)r, 4);
    if (s.suppressor)
      std::memcpy(stage + stage_supp_offset(s, n) + 4u * (size_t)kSuppRowFloats * i, b + blob_supp_offset(s), 4u * (size_t)kSuppRowFloats);
  }
}

}  // namespace sstate
}  // namespace af
